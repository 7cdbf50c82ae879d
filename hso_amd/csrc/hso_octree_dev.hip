// hso_octree_dev.hip — the oct-tree distribution of hso_octree.cpp on gfx950: one workgroup per key set (one keyframe),
// byte for byte the selection of hso_gpu_select_octree (which stays the definition; reference
// src/feature_detection.cpp:833-1122).
//
// What makes the host's list walk parallel:
//   * the keys of a node are always in ascending input index (the column fill goes in input order, every split is a
//     stable partition), so nothing is partitioned: every key carries the list position of its node (node_of[]), and a
//     split is four counters per node + one pass over the keys;
//   * the node list is an array in list order.  A round removes the nodes it splits and pushes their non-empty children
//     to the front one by one, so afterwards the list is [children in reverse creation order | the other nodes in their
//     old order]: two prefix sums.  In a sweep (first phase) the creation order is list order x quadrant; in the second
//     phase it is the order of the host's sort — key count descending, then creation id descending, i.e. list
//     position ascending among this round's children — x quadrant, cut at the first prefix that reaches n_features.
// Per round: zero counters, count quadrants (global atomics), rank / scan, write the new list into the other buffer,
// re-label the keys.  The final pick per node is two atomic passes: lowest species (+ "holds an occupancy key"), then a
// 64-bit minimum over (response descending, input index ascending) among the keys of that species.
//
// Everything a set needs beyond LDS (labels, two list buffers, counters) is global scratch that stays in L2; only the
// second phase's sort keys are in LDS, which is what bounds n_features (HSO_OCTREE_MAX_FEATURES).  Counters that
// atomics update are read and written with agent-scope atomic accesses only, so no plain load can meet a stale L1 line.
#include "hso_octree_dev.h"
#include "hso_wave.h"
#include <cmath>

#define OCT_THREADS 1024

struct OctNode { int x0, y0, x1, y1, cnt, exp; };   // exp: a multi-key child of the round that made it (the host's `expandable`)

struct OctArgs {
  const hso_keypoint* keys; const int* key_begin;
  int* node_of;                      // [total keys]: list position of the key's node
  char* work; size_t per_set;        // per set: [list A | list B | counters 4 x ncap | cbase | split]
  int ncap, n_ini; float hX;
  int min_y, max_y, n_features;
  hso_keypoint* out; int out_cap; int* n_out;
};

__device__ __forceinline__ int oct_ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void oct_st(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// exclusive prefix of v over the workgroup's threads (all call); total = the sum
__device__ __forceinline__ int oct_scan(int v, int* s_w, int& total)
{
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int inc = hso_dev::wave_inclusive_scan(v, lane);
  if (lane == 63) s_w[wv] = inc;
  __syncthreads();
  int before = 0, tot = 0;
#pragma unroll
  for (int k = 0; k < OCT_THREADS / 64; k++) { const int w = s_w[k]; before += k < wv ? w : 0; tot += w; }
  __syncthreads();
  total = tot;
  return before + inc - v;
}

// ExtractorNode::DivideNode's midpoints and the quadrant of a key (hso_octree.cpp: Tree::divide)
__device__ __forceinline__ void oct_mid(const OctNode& nd, int& mx, int& my)
{
  mx = nd.x0 + (int)ceilf((float)(nd.x1 - nd.x0) / 2);
  my = nd.y0 + (int)ceilf((float)(nd.y1 - nd.y0) / 2);
}
__device__ __forceinline__ int oct_quad(const OctNode& nd, float x, float y)
{
  int mx, my;
  oct_mid(nd, mx, my);
  return (x < (float)mx ? 0 : 1) + (y < (float)my ? 0 : 2);
}

__global__ __launch_bounds__(OCT_THREADS) void k_octree(OctArgs A)
{
  __shared__ int s_w[OCT_THREADS / 64];
  __shared__ int s_col[HSO_OCTREE_MAX_COLUMNS], s_colpos[HSO_OCTREE_MAX_COLUMNS];
  __shared__ int s_sz[HSO_OCTREE_MAX_FEATURES], s_ord[HSO_OCTREE_MAX_FEATURES];
  __shared__ int s_L, s_nexp;
  const int set = blockIdx.x, t = threadIdx.x;
  const int kb = A.key_begin[set], n = A.key_begin[set + 1] - kb;
  if (n <= 0) { if (t == 0) A.n_out[set] = 0; return; }
  const hso_keypoint* keys = A.keys + kb;
  int* node_of = A.node_of + kb;
  char* w = A.work + (size_t)set * A.per_set;
  const int ncap = A.ncap;
  OctNode* cur = reinterpret_cast<OctNode*>(w);
  OctNode* nxt = cur + ncap;
  int* cc = reinterpret_cast<int*>(nxt + ncap);     // [ncap][4]
  int* cbase = cc + 4 * (size_t)ncap;               // creation index of a split node's first child
  int* split = cbase + ncap;
  const int n_features = A.n_features;

  // ---- the initial column nodes, keys in input order
  if (t < HSO_OCTREE_MAX_COLUMNS) s_col[t] = 0;
  __syncthreads();
  int bad = 0;
  for (int i = t; i < n; i += OCT_THREADS) {
    const int x = (int)keys[i].x;
    const int c = (int)((float)x / A.hX);
    if (c < 0 || c >= A.n_ini) bad = 1;
    else { atomicAdd(&s_col[c], 1); node_of[i] = c; }
  }
  bad = __syncthreads_or(bad);
  if (bad) { if (t == 0) A.n_out[set] = HSO_E_INVALID; return; }    // out-of-range write in the reference
  if (t == 0) {
    int pos = 0;
    for (int c = 0; c < A.n_ini; c++) {
      if (s_col[c] == 0) continue;                                   // empty initial nodes are erased
      s_colpos[c] = pos;
      cur[pos++] = OctNode{(int)(A.hX * (float)c), A.min_y, (int)(A.hX * (float)(c + 1)), A.max_y, s_col[c], 0};
    }
    s_L = pos;
  }
  __syncthreads();
  for (int i = t; i < n; i += OCT_THREADS) node_of[i] = s_colpos[node_of[i]];
  int L = s_L, phase2 = 0, c_prev = 0, fail = 0;
  __syncthreads();

  for (;;) {
    // ---- quadrant counts of the nodes this round may split: every multi-key node in a sweep, last round's multi-key children after
    for (int i = t; i < 4 * L; i += OCT_THREADS) oct_st(&cc[i], 0);
    if (t == 0) s_nexp = 0;
    __syncthreads();
    for (int i = t; i < n; i += OCT_THREADS) {
      const int p = node_of[i];
      const OctNode nd = cur[p];
      if (phase2 ? nd.exp != 0 : nd.cnt > 1) atomicAdd(&cc[4 * p + oct_quad(nd, keys[i].x, keys[i].y)], 1);
    }
    __syncthreads();
    // ---- which nodes are split, and the creation index of their first child
    int C = 0;
    if (!phase2) {
      for (int base = 0; base < L; base += OCT_THREADS) {
        const int p = base + t;
        int v = 0;
        const bool sp = p < L && cur[p].cnt > 1;
        if (sp) for (int q = 0; q < 4; q++) v += oct_ld(&cc[4 * p + q]) > 0;
        int tot;
        const int e = oct_scan(v, s_w, tot);
        if (p < L) { cbase[p] = C + e; split[p] = sp; }
        C += tot;
      }
    } else {
      // the host sorts (key count, creation id) and takes from the back: larger count first, among equals the younger node — the one
      // nearer the list's head.  Rank by counting; the candidates are among the c_prev children at the head of the list.
      for (int p = t; p < L; p += OCT_THREADS) split[p] = 0;
      for (int p = t; p < c_prev; p += OCT_THREADS) s_sz[p] = cur[p].exp ? cur[p].cnt : 0;
      __syncthreads();
      int mine = 0;
      for (int p = t; p < c_prev; p += OCT_THREADS) {
        const int sz = s_sz[p];
        if (sz == 0) continue;
        int r = 0;
        for (int j = 0; j < c_prev; j++) { const int sj = s_sz[j]; r += (sj > sz) || (sj == sz && j < p); }
        s_ord[r] = p;
        mine++;
      }
      int T;
      (void)oct_scan(mine, s_w, T);     // (its barriers also publish s_ord)
      for (int base = 0; base < T; base += OCT_THREADS) {
        const int r = base + t;
        int v = 0, p = 0;
        if (r < T) { p = s_ord[r]; for (int q = 0; q < 4; q++) v += oct_ld(&cc[4 * p + q]) > 0; }
        int tot;
        const int e = oct_scan(v, s_w, tot);
        // the list holds L + (C + e) - r nodes when the host reaches candidate r; it stops once that is n_features or more
        const bool sp = r < T && L + (C + e) - r < n_features;
        if (sp) { cbase[p] = C + e; split[p] = 1; }
        int tot_split;
        (void)oct_scan(sp ? v : 0, s_w, tot_split);
        C += tot_split;
        if (tot_split != tot) break;      // the cut (uniform: every thread holds the same totals)
      }
      __syncthreads();
    }
    // ---- the new list: children in reverse creation order, then the nodes that stay, in their order
    int S = 0;
    for (int base = 0; base < L; base += OCT_THREADS) { const int p = base + t; S += __syncthreads_count(p < L && !split[p]); }
    const int L_new = C + S;
    if (L_new > ncap || (phase2 && c_prev > HSO_OCTREE_MAX_FEATURES)) { fail = 1; break; }
    int keep = 0, nexp = 0;
    for (int base = 0; base < L; base += OCT_THREADS) {
      const int p = base + t;
      const bool stay = p < L && !split[p];
      int tot;
      const int e = oct_scan(stay, s_w, tot);
      if (p < L) {
        OctNode nd = cur[p];
        if (stay) {
          const int np = C + keep + e;
          nd.exp = 0;
          nxt[np] = nd;
          oct_st(&cc[4 * p], np);
        } else {
          int mx, my;
          oct_mid(nd, mx, my);
          int j = cbase[p];
          for (int q = 0; q < 4; q++) {
            const int c = oct_ld(&cc[4 * p + q]);
            if (c == 0) continue;
            const int np = C - 1 - j++;
            nxt[np] = OctNode{(q & 1) ? mx : nd.x0, (q & 2) ? my : nd.y0, (q & 1) ? nd.x1 : mx, (q & 2) ? nd.y1 : my, c, c > 1};
            oct_st(&cc[4 * p + q], np);
            nexp += c > 1;
          }
        }
      }
      keep += tot;
    }
    if (nexp) atomicAdd(&s_nexp, nexp);
    __syncthreads();
    for (int i = t; i < n; i += OCT_THREADS) {
      const int p = node_of[i];
      const OctNode nd = cur[p];
      node_of[i] = oct_ld(&cc[4 * p + (split[p] ? oct_quad(nd, keys[i].x, keys[i].y) : 0)]);
    }
    const int n_to_expand = s_nexp;
    __syncthreads();
    { OctNode* x = cur; cur = nxt; nxt = x; }
    const int L_old = L;
    L = L_new;
    if (L >= n_features || L == L_old) break;
    if (!phase2 && L + n_to_expand * 3 > n_features) phase2 = 1;
    c_prev = C;
    if (phase2 && c_prev > HSO_OCTREE_MAX_FEATURES) { fail = 1; break; }
  }
  if (fail) { if (t == 0) A.n_out[set] = HSO_E_UNSUPPORTED; return; }

  // ---- one key per node: lowest species, then highest response, then first in input order; a node with an occupancy key yields nothing
  unsigned long long* best = reinterpret_cast<unsigned long long*>(cc);    // node p: cc[4p] species, cc[4p + 1] occupancy, best[2p + 1]
  for (int p = t; p < L; p += OCT_THREADS) {
    oct_st(&cc[4 * p], 0x7fffffff); oct_st(&cc[4 * p + 1], 0);
    __hip_atomic_store(&best[2 * p + 1], ~0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  for (int i = t; i < n; i += OCT_THREADS) {
    const int p = node_of[i], sp = keys[i].species;
    if (sp == HSO_KP_OCCUR) atomicOr(&cc[4 * p + 1], 1);
    atomicMin(&cc[4 * p], sp);
  }
  __syncthreads();
  for (int i = t; i < n; i += OCT_THREADS) {
    const int p = node_of[i];
    if (keys[i].species != oct_ld(&cc[4 * p])) continue;
    const float r = keys[i].response + 0.0f;                     // -0 -> +0: the host compares them equal
    const unsigned u = __float_as_uint(r);
    const unsigned asc = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    atomicMin(&best[2 * p + 1], ((unsigned long long)(~asc) << 32) | (unsigned)i);
  }
  __syncthreads();
  int n_sel = 0;
  hso_keypoint* out = A.out + (size_t)set * A.out_cap;
  for (int base = 0; base < L; base += OCT_THREADS) {
    const int p = base + t;
    const bool emit = p < L && oct_ld(&cc[4 * p + 1]) == 0;
    int tot;
    const int e = oct_scan(emit, s_w, tot);
    if (emit && n_sel + e < A.out_cap) {
      const unsigned idx = (unsigned)__hip_atomic_load(&best[2 * p + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      out[n_sel + e] = keys[idx];
    }
    n_sel += tot;
  }
  if (t == 0) A.n_out[set] = n_sel;
}

int hso_octree_plan(hso_gpu_ctx* ctx, int min_x, int max_x, int min_y, int max_y, int n_features, OctreePlan* plan)
{
  if (max_x <= min_x || max_y <= min_y) return hso_fail(ctx, HSO_E_INVALID, "select_octree: empty rectangle");
  const int nIni = (int)std::round((float)(max_x - min_x) / (max_y - min_y));
  if (nIni < 1) return hso_fail(ctx, HSO_E_INVALID, "select_octree: rectangle more than twice as high as wide");
  if (nIni > HSO_OCTREE_MAX_COLUMNS || n_features > HSO_OCTREE_MAX_FEATURES)
    return hso_fail(ctx, HSO_E_UNSUPPORTED, "select_octree: n_features or width / height beyond what the device kernel takes");
  plan->n_ini = nIni;
  plan->hX = (float)(max_x - min_x) / nIni;
  plan->min_y = min_y; plan->max_y = max_y; plan->n_features = n_features;
  // a sweep runs only while it cannot pass n_features (list + 3 per multi-key child <= n_features), except the first (4 per column);
  // the second phase stops within 3 of n_features
  plan->ncap = std::max(std::max(n_features, 0) + 3, 4 * nIni) + 5;
  plan->per_set = hso_al256((sizeof(OctNode) * 2 + sizeof(int) * 6) * (size_t)plan->ncap);
  return HSO_OK;
}

size_t hso_octree_scratch_bytes(const OctreePlan& plan, int n_sets, size_t total_keys)
{
  return hso_al256(sizeof(int) * total_keys) + plan.per_set * (size_t)n_sets;
}

int hso_octree_reserve(hso_gpu_ctx* ctx, size_t bytes, char** d)
{
  if (int rc = hso_dev_reserve(ctx, ctx->stream, &ctx->d_octree, &ctx->octree_cap, bytes)) return rc;   // (bytes > 0: both callers' tables are never empty)
  *d = ctx->d_octree;
  return HSO_OK;
}

int hso_octree_launch(hso_gpu_ctx* ctx, const OctreePlan& plan, const hso_keypoint* d_keys, const int* d_key_begin, int n_sets, size_t total_keys,
                      hso_keypoint* d_out, int out_cap, int* d_n_out, char* d_scratch)
{
  OctArgs A;
  A.keys = d_keys; A.key_begin = d_key_begin;
  A.node_of = reinterpret_cast<int*>(d_scratch);
  A.work = d_scratch + hso_al256(sizeof(int) * total_keys); A.per_set = plan.per_set;
  A.ncap = plan.ncap; A.n_ini = plan.n_ini; A.hX = plan.hX;
  A.min_y = plan.min_y; A.max_y = plan.max_y; A.n_features = plan.n_features;
  A.out = d_out; A.out_cap = out_cap; A.n_out = d_n_out;
  hipLaunchKernelGGL(k_octree, dim3(n_sets), dim3(OCT_THREADS), 0, ctx->stream, A);
  HSO_HIP_CHECK(ctx, hipGetLastError());
  return HSO_OK;
}

extern "C" int hso_gpu_select_octree_batch(hso_gpu_ctx* ctx, const hso_keypoint* keys, const int32_t* key_begin, int n_sets,
                                           int min_x, int max_x, int min_y, int max_y, int n_features,
                                           hso_keypoint* out, int out_cap, int32_t* n_out)
{
  if (!ctx) return HSO_E_INVALID;
  if (n_sets < 0 || out_cap < 0 || (n_sets > 0 && (!key_begin || !n_out)) || (n_sets > 0 && out_cap > 0 && !out))
    return hso_fail(ctx, HSO_E_INVALID, "select_octree_batch: bad argument");
  if (n_sets == 0) return HSO_OK;
  if (key_begin[0] != 0) return hso_fail(ctx, HSO_E_INVALID, "select_octree_batch: key_begin[0] must be 0");
  for (int i = 0; i < n_sets; i++)
    if (key_begin[i + 1] < key_begin[i]) return hso_fail(ctx, HSO_E_INVALID, "select_octree_batch: key_begin must not decrease");
  const size_t total = (size_t)key_begin[n_sets];
  if (total > 0 && !keys) return hso_fail(ctx, HSO_E_INVALID, "select_octree_batch: bad argument");
  OctreePlan plan;
  if (int rc = hso_octree_plan(ctx, min_x, max_x, min_y, max_y, n_features, &plan)) return rc;
  HSO_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const size_t o_begin = 0, o_nout = hso_al256(sizeof(int) * ((size_t)n_sets + 1)), o_keys = o_nout + hso_al256(sizeof(int) * (size_t)n_sets);
  const size_t o_out = o_keys + hso_al256(sizeof(hso_keypoint) * total), o_scratch = o_out + hso_al256(sizeof(hso_keypoint) * (size_t)n_sets * out_cap);
  char* d = nullptr;
  if (int rc = hso_octree_reserve(ctx, o_scratch + hso_octree_scratch_bytes(plan, n_sets, total), &d)) return rc;
  HSO_HIP_CHECK(ctx, hipMemcpyAsync(d + o_begin, key_begin, sizeof(int) * ((size_t)n_sets + 1), hipMemcpyHostToDevice, ctx->stream));
  if (total > 0) HSO_HIP_CHECK(ctx, hipMemcpyAsync(d + o_keys, keys, sizeof(hso_keypoint) * total, hipMemcpyHostToDevice, ctx->stream));
  if (int rc = hso_octree_launch(ctx, plan, reinterpret_cast<const hso_keypoint*>(d + o_keys), reinterpret_cast<const int*>(d + o_begin), n_sets, total,
                                 reinterpret_cast<hso_keypoint*>(d + o_out), out_cap, reinterpret_cast<int*>(d + o_nout), d + o_scratch))
    return rc;
  HSO_HIP_CHECK(ctx, hipMemcpyAsync(n_out, d + o_nout, sizeof(int) * (size_t)n_sets, hipMemcpyDeviceToHost, ctx->stream));
  if (out_cap > 0)
    HSO_HIP_CHECK(ctx, hipMemcpyAsync(out, d + o_out, sizeof(hso_keypoint) * (size_t)n_sets * out_cap, hipMemcpyDeviceToHost, ctx->stream));
  HSO_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return HSO_OK;
}
