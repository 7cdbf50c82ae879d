// hso_klt_ranges.h — the row ranges of hso_gpu_klt_track_multi: the check of the pair table against the concatenated point tables
// and the per-row pair index the upload carries.  Plain host code without a HIP include, so that a stand-alone program can run
// it under a sanitizer (tests/klt_tables_main.cpp).
#pragma once
#include <stdint.h>
#include <algorithm>
#include <vector>
#include "../../include/hso_gpu.h"

// Every pair owns rows first .. first + n - 1, all of them inside 0 .. n_total - 1, and no row has two owners; a pair with n = 0
// owns nothing and collides with nobody (0 <= first <= n_total is all that is asked of it).  HSO_OK: `active` holds the pairs with
// n > 0 in the caller's order.  HSO_E_INVALID otherwise.
inline int hso_klt_check_ranges(const hso_klt_pair* pairs, int n_pairs, int n_total, std::vector<int32_t>& active)
{
  active.clear();
  if (n_pairs < 0 || n_total < 0 || (n_pairs > 0 && !pairs)) return HSO_E_INVALID;
  for (int p = 0; p < n_pairs; p++) {
    if (pairs[p].first < 0 || pairs[p].n < 0 || (int64_t)pairs[p].first + pairs[p].n > (int64_t)n_total) return HSO_E_INVALID;
    if (pairs[p].n > 0) active.push_back(p);
  }
  std::vector<int32_t> by_first(active);
  std::sort(by_first.begin(), by_first.end(), [&](int32_t a, int32_t b) { return pairs[a].first < pairs[b].first; });
  for (size_t i = 1; i < by_first.size(); i++) {
    const hso_klt_pair& a = pairs[by_first[i - 1]];
    if ((int64_t)a.first + a.n > (int64_t)pairs[by_first[i]].first) return HSO_E_INVALID;
  }
  return HSO_OK;
}

// pair_of[row] = index into `active` of the row's owner, -1 for a row nobody owns (ranges checked by hso_klt_check_ranges)
inline void hso_klt_fill_pair_of(const hso_klt_pair* pairs, const std::vector<int32_t>& active, int n_total, int32_t* pair_of)
{
  std::fill(pair_of, pair_of + n_total, -1);
  for (size_t a = 0; a < active.size(); a++) {
    const hso_klt_pair& p = pairs[active[a]];
    std::fill(pair_of + p.first, pair_of + p.first + p.n, (int32_t)a);
  }
}
