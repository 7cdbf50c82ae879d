// hso_klt_batch.h — the tables of one hso_gpu_klt_track_multi call as the engine builds them: the point lists of the sequences
// that continue their two-view initialisation, concatenated, with one hso_klt_pair per sequence; and the slices a sequence reads
// its results from.  Plain host code over include/hso_gpu.h alone (no engine type, no device), so that a stand-alone program can
// run it under a sanitizer (tests/klt_tables_main.cpp).
#pragma once
#include <stdint.h>
#include <stdexcept>
#include <vector>
#include "../../include/hso_gpu.h"

namespace hso {
namespace engine {

struct KltBatch {
  std::vector<hso_klt_pair> pairs;
  std::vector<float> px_prev, px_init;          // 2 floats per row
  std::vector<hso_klt_result> res;              // one per row, sized by finish()

  // one sequence: px[i][0], px[i][1] for i < n are its points in the previous frame, and the initial flow's targets as well
  // (px_prev_ = the positions in the previous frame; while only the reference has been seen both are the reference's).
  // Returns the sequence's pair.
  template <class Points> int add(int64_t frame_prev, int64_t frame_cur, const Points& px, size_t n)
  {
    const size_t first = px_prev.size() / 2;
    if (first + n > (size_t)INT32_MAX) throw std::length_error("klt batch: more rows than the call's int32 counts hold");
    pairs.push_back(hso_klt_pair{frame_prev, frame_cur, (int32_t)first, (int32_t)n});
    px_prev.reserve(2 * (first + n)); px_init.reserve(2 * (first + n));
    for (size_t i = 0; i < n; i++) {
      const float x = (float)px[i][0], y = (float)px[i][1];
      px_prev.push_back(x); px_prev.push_back(y);
      px_init.push_back(x); px_init.push_back(y);
    }
    return (int)pairs.size() - 1;
  }
  void finish() { res.assign(px_prev.size() / 2, hso_klt_result{}); }
  int n_total() const { return (int)(px_prev.size() / 2); }
  // pair p's slices (a pair without rows: pointers one past the tables' ends at most, never dereferenced)
  size_t rows(int p) const { return (size_t)pairs[(size_t)p].n; }
  const float* prev_of(int p) const { return px_prev.data() + 2 * (size_t)pairs[(size_t)p].first; }
  const float* init_of(int p) const { return px_init.data() + 2 * (size_t)pairs[(size_t)p].first; }
  hso_klt_result* res_of(int p) { return res.data() + (size_t)pairs[(size_t)p].first; }
};

}  // namespace engine
}  // namespace hso
