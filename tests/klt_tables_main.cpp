// klt_tables_main.cpp — the host half of the batched KLT call, run on its own (tests/test_klt_multi_cpu.py builds it with
// -fsanitize=address,undefined): the engine's table concatenation (hso_amd/host/hso_klt_batch.h) and the device library's range
// checks and per-row pair index (hso_amd/csrc/hso_klt_ranges.h).  Neither needs a device.  Prints "ok" and returns 0, or says
// what failed and returns 1.
#include <array>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../hso_amd/csrc/hso_klt_ranges.h"
#include "../hso_amd/host/hso_klt_batch.h"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

static int check(const std::vector<hso_klt_pair>& pairs, int n_total, std::vector<int32_t>* active_out = nullptr)
{
  std::vector<int32_t> active;
  const int rc = hso_klt_check_ranges(pairs.data(), (int)pairs.size(), n_total, active);
  if (active_out) *active_out = active;
  return rc;
}

int main()
{
  using hso::engine::KltBatch;
  // ---- concatenation: three sequences, the middle one without points
  const size_t counts[3] = {37, 0, 300};
  std::vector<std::vector<std::array<double, 2>>> px(3);
  for (int s = 0; s < 3; s++)
    for (size_t i = 0; i < counts[s]; i++) px[(size_t)s].push_back({100.0 * s + (double)i + 0.25, 7.0 * s + 0.5 * (double)i});
  KltBatch B;
  for (int s = 0; s < 3; s++) EXPECT(B.add(10 + s, 20 + s, px[(size_t)s], px[(size_t)s].size()) == s);
  B.finish();
  EXPECT(B.n_total() == 337 && B.res.size() == 337 && B.px_prev.size() == 674 && B.px_init.size() == 674);
  EXPECT(B.pairs[0].first == 0 && B.pairs[0].n == 37 && B.pairs[1].first == 37 && B.pairs[1].n == 0 && B.pairs[2].first == 37 && B.pairs[2].n == 300);
  for (int s = 0; s < 3; s++) {
    EXPECT(B.pairs[(size_t)s].frame_prev == 10 + s && B.pairs[(size_t)s].frame_cur == 20 + s && B.rows(s) == counts[s]);
    for (size_t i = 0; i < counts[s]; i++) {
      EXPECT(B.prev_of(s)[2 * i] == (float)px[(size_t)s][i][0] && B.prev_of(s)[2 * i + 1] == (float)px[(size_t)s][i][1]);
      EXPECT(B.init_of(s)[2 * i] == B.prev_of(s)[2 * i] && B.init_of(s)[2 * i + 1] == B.prev_of(s)[2 * i + 1]);
    }
    for (size_t i = 0; i < counts[s]; i++) B.res_of(s)[i].status = s + 1;       // every row of a slice is writable, and only its own
  }
  for (size_t r = 0; r < 337; r++) EXPECT(B.res[r].status == (r < 37 ? 1 : 3));
  // what the engine built passes the device library's checks
  std::vector<int32_t> active;
  EXPECT(check(B.pairs, B.n_total(), &active) == HSO_OK && active.size() == 2 && active[0] == 0 && active[1] == 2);
  std::vector<int32_t> pair_of(337, 99);
  hso_klt_fill_pair_of(B.pairs.data(), active, 337, pair_of.data());
  for (size_t r = 0; r < 337; r++) EXPECT(pair_of[r] == (r < 37 ? 0 : 1));
  // an empty batch
  KltBatch E;
  E.finish();
  EXPECT(E.n_total() == 0 && check(E.pairs, 0) == HSO_OK);

  // ---- range checks
  const hso_klt_pair a{1, 2, 300, 37}, none{1, 2, 300, 0}, c{2, 3, 0, 300};
  EXPECT(check({a, none, c}, 337, &active) == HSO_OK && active.size() == 2 && active[0] == 0 && active[1] == 2);   // any order of `first`
  pair_of.assign(340, 99);
  hso_klt_fill_pair_of(std::vector<hso_klt_pair>{a, none, c}.data(), active, 337, pair_of.data());
  for (size_t r = 0; r < 337; r++) EXPECT(pair_of[r] == (r < 300 ? 1 : 0));
  EXPECT(pair_of[337] == 99 && pair_of[339] == 99);                                                              // nothing beyond n_total
  EXPECT(check({a, c}, 336) == HSO_E_INVALID);                                                                    // past the tables' end
  EXPECT(check({{1, 2, 0, 12}, {1, 2, 11, 9}}, 20) == HSO_E_INVALID);                                             // overlap by one row
  EXPECT(check({{1, 2, 11, 9}, {1, 2, 0, 12}}, 20) == HSO_E_INVALID);                                             // the same, other order
  EXPECT(check({{1, 2, 0, 11}, {1, 2, 11, 9}}, 20) == HSO_OK);                                                    // adjacent
  EXPECT(check({{1, 2, 5, 3}, {1, 2, 5, 3}}, 20) == HSO_E_INVALID);                                               // the same rows twice
  EXPECT(check({{1, 2, -1, 3}}, 20) == HSO_E_INVALID && check({{1, 2, 0, -3}}, 20) == HSO_E_INVALID);
  EXPECT(check({{1, 2, 2147483647, 2147483647}}, 2147483647) == HSO_E_INVALID);                                   // first + n does not wrap
  EXPECT(check({{1, 2, 20, 0}}, 20) == HSO_OK && check({{1, 2, 21, 0}}, 20) == HSO_E_INVALID);
  // a gap: rows nobody owns are marked
  EXPECT(check({{1, 2, 10, 5}}, 20, &active) == HSO_OK);
  pair_of.assign(20, 99);
  const hso_klt_pair gap{1, 2, 10, 5};
  hso_klt_fill_pair_of(&gap, active, 20, pair_of.data());
  for (size_t r = 0; r < 20; r++) EXPECT(pair_of[r] == (r >= 10 && r < 15 ? 0 : -1));
  std::vector<int32_t> unused;
  EXPECT(hso_klt_check_ranges(nullptr, 1, 5, unused) == HSO_E_INVALID && hso_klt_check_ranges(nullptr, 0, 5, unused) == HSO_OK);
  if (failures) return 1;
  std::puts("ok");
  return 0;
}
