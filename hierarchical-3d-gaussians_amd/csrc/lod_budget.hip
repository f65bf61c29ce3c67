// Budget-exact hierarchy cut (opt-in, beside hgs_lod_cut_view of lod_frustum.hip): the finest granularity
// tau* >= tau_min whose cut costs at most `budget`, and the cut at tau*, in ONE call with one host wait.
//
// The rule (include/hgs.h "Budget-exact cut"; tests/budget_cut_spec.py restates it).  When the
// boxes nest, the cost of the cut at tau is a sum over nodes of indicator functions of tau.  With s_n = node_size(n),
// s_par the parent's (+inf at the root), L, M the node's count_leafs / count_merged and k_n = "the entry of n survives
// the frustum cull" (independent of tau):
//   entries(tau) = sum_n k_n ([s_par >= tau] (L + M) - [s_n >= tau] M)
//   parents(tau) = #{p : s_p / 2 < tau <= s_p and m_p < tau},  m_p = min s_c over p's kept children that own rows
//   rows(tau)    = entries(tau) + parents(tau)
// i.e. cost(tau) = sum of the values of the EVENTS (key, value) with key >= tau: (s_par, +(L + M) k), (s_n, -M k) per
// node and, for rows, (s_p, +1), (max(s_p / 2, m_p), -1) per parent whose second key is below the first.  Keys are
// float32 bit patterns of non-negative numbers, which order as integers, so "the finest tau that fits" is a weighted
// selection over 31-bit keys: a radix descent of three digits (11, 10, 10 bits; shifts 20, 10, 0), one histogram pass
// over the nodes and one one-workgroup pick per digit, lo / hi / cost(hi) staying in device memory.  All sums are
// integer adds: the result is exact and two calls give the same bits.
//
// Layout: size pass (s_n and k_n in 4 bytes per node: the later passes gather 4 bytes instead of a 32-byte box and a
// 16-byte ball), parent-event pass (rows only), 3 x (histogram, pick), then mark / scan / emit as lod_frustum.hip with
// tau* read from device memory: the rules and the parts of those passes are lod_cut.h's.
#include "lod_cut.h"
#include <string.h>

namespace hgs {
namespace {

constexpr uint32_t kInfBits = 0x7F800000u;
constexpr uint32_t kKeyMask = 0x7FFFFFFFu;
constexpr uint32_t kNoEvent = 0xFFFFFFFFu;
constexpr int kBins = 2048;                 // the first digit has (0x7F800000 >> 20) = 2040 boundaries, the others 1024
constexpr int kHistGrid = 2048;             // workgroups of a histogram pass (grid-stride over the nodes)
constexpr uint32_t kTauCapacity = 0xFFFFFFFFu;   // result word 2: the coarsest cut exceeds the budget
constexpr uint32_t kTauBadInput = 0xFFFFFFFEu;   //                a size that is negative or NaN, or sizes that do not nest

// state words (device memory, behind the histogram)
enum { S_LO = 0, S_HI, S_COST_HI, S_FIRST, S_DONE, S_FAIL, S_BAD, S_PAD, S_RESULT /* kept, unculled, tau bits, cost */,
       S_WORDS = 12 };

// Size pass, one thread per node: sk[n] = bits(s_n) | k_n << 31.  Its first thread sets the bracket of the descent (the
// histogram and the other state words were zeroed by the memset in front).  A node record that points outside the node
// list, negative counts and a size that is negative or NaN set S_BAD: the call then fails without writing an output.
__global__ __launch_bounds__(256) void budget_size_kernel(const int32_t* __restrict__ nodes,
                                                          const float* __restrict__ boxes,
                                                          const float4* __restrict__ bounds, int N, Vec3 vp, Frustum f,
                                                          uint32_t tau_min_bits, uint32_t* __restrict__ sk,
                                                          uint32_t* __restrict__ state) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    state[S_LO] = tau_min_bits;
    state[S_HI] = kInfBits;
    state[S_FIRST] = 1u;
  }
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  const int32_t* nd = nodes + (size_t)n * kNodeInts;
  const int par = nd[1], nch = nd[6];
  const long long c0 = nd[5];
  bool bad = par >= N || nd[3] < 0 || nd[4] < 0 || nch < 0 || (nch > 0 && (c0 < 0 || c0 + nch > (long long)N));
  const float s = node_size(boxes, n, vp);
  bad |= !(s >= 0.0f);
  const bool kept = bad || bounds == nullptr || !entry_culled(bounds, n, par, f);
  sk[n] = (__float_as_uint(s) & kKeyMask) | (kept ? 0x80000000u : 0u);
  if (bad) state[S_BAD] = 1u;         // (benign race: every writer stores 1)
}

// Parent-event pass (cost = rows), one thread per node: ev[p] = the key of p's -1 event, max(s_p / 2, m_p), when p has
// a kept child that owns rows and that key is below s_p; else kNoEvent.  Also the view's own nesting check: a child
// larger than its parent sets S_BAD.
__global__ __launch_bounds__(256) void budget_parent_kernel(const int32_t* __restrict__ nodes,
                                                            const uint32_t* __restrict__ sk, int N,
                                                            uint32_t* __restrict__ ev, uint32_t* __restrict__ bad) {
#pragma clang fp contract(off)
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= N) return;
  if (*bad) { ev[p] = kNoEvent; return; }      // (a record may point anywhere: do not follow it)
  const int32_t* nd = nodes + (size_t)p * kNodeInts;
  const int c0 = nd[5], nch = nd[6];
  const uint32_t sp_bits = sk[p] & kKeyMask;
  uint32_t m = kNoEvent;
  bool unnested = false;
  for (int k = 0; k < nch; ++k) {
    const int c = c0 + k;
    const uint32_t w = sk[c];
    const int32_t* cd = nodes + (size_t)c * kNodeInts;
    unnested |= (w & kKeyMask) > sp_bits;
    if ((w >> 31) && cd[3] + cd[4] > 0) m = min(m, w & kKeyMask);
  }
  uint32_t e = kNoEvent;
  if (m != kNoEvent) {
    const uint32_t half = __float_as_uint(0.5f * __uint_as_float(sp_bits));
    const uint32_t key = max(half, m);
    if (key < sp_bits) e = key;
  }
  ev[p] = e;
  if (unnested) *bad = 1u;
}

// (bin, value) of one event for the current digit, or value 0 when the event plays no part: bin q(x) = (x >> sh) -
// (lo >> sh) for lo <= x < hi -- bin 0 holds [lo, first boundary) and only matters in the first pass, where it decides
// "the request fits" -- and bin Q = q(hi) for x >= hi in the first pass (later, those events are part of cost(hi)).
__device__ __forceinline__ void place(uint32_t key, int32_t val, uint32_t lo, uint32_t hi, int sh, bool first,
                                      uint32_t& bin, int32_t& v) {
  const bool in = key >= lo && (key < hi || first);
  bin = (min(key, hi) >> sh) - (lo >> sh);
  v = in ? val : 0;
}

// add v to bins[bin] for the lanes with v != 0.  Node sizes cluster in a few exponents, so at the first digit many
// lanes of a wave hit one bin: two rounds of "the lanes that share the first active lane's bin add up in registers and
// one of them adds to LDS", then plain LDS adds for what is left.
__device__ __forceinline__ void wave_add(uint32_t* bins, uint32_t bin, int32_t v) {
  bool active = v != 0;
#pragma unroll
  for (int round = 0; round < 2; ++round) {
    const unsigned long long live = __ballot(active);
    if (live == 0ull) return;
    const int leader = __ffsll((long long)live) - 1;
    const uint32_t lbin = (uint32_t)__shfl((int)bin, leader, 64);
    const bool mine = active && bin == lbin;
    int32_t sum = mine ? v : 0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
    if ((int)(threadIdx.x & 63) == leader && sum != 0) atomicAdd(&bins[lbin], (uint32_t)sum);
    active = active && !mine;
  }
  if (active) atomicAdd(&bins[bin], (uint32_t)v);
}

// Histogram pass of one digit (shift sh), grid-stride over the nodes: every thread generates its node's events and adds
// those inside the current bracket to the workgroup's LDS histogram; the non-zero bins then go to the global one.
__global__ __launch_bounds__(256) void budget_hist_kernel(const int32_t* __restrict__ nodes,
                                                          const uint32_t* __restrict__ sk,
                                                          const uint32_t* __restrict__ ev, int N, int sh, int rows,
                                                          uint32_t* __restrict__ hist,
                                                          const uint32_t* __restrict__ state) {
  __shared__ uint32_t bins[kBins];
  if (state[S_DONE] | state[S_FAIL] | state[S_BAD]) return;
  const uint32_t lo = state[S_LO], hi = state[S_HI];
  const bool first = state[S_FIRST] != 0u;
  for (int t = threadIdx.x; t < kBins; t += 256) bins[t] = 0u;
  __syncthreads();
  // (whole waves stay in the loop: wave_add shuffles)
  const int n_round = (N + 255) / 256 * 256;
  for (int n = blockIdx.x * 256 + threadIdx.x; n < n_round; n += gridDim.x * 256) {
    uint32_t b0 = 0, b1 = 0, b2 = 0, b3 = 0;
    int32_t v0 = 0, v1 = 0, v2 = 0, v3 = 0;
    if (n < N) {
      const int32_t* nd = nodes + (size_t)n * kNodeInts;
      const int par = nd[1];
      const int32_t L = nd[3], M = nd[4];
      const uint32_t w = sk[n];
      const uint32_t key = w & kKeyMask;
      const int32_t k = (int32_t)(w >> 31);
      const uint32_t pkey = par >= 0 ? (sk[par] & kKeyMask) : kInfBits;
      place(pkey, (L + M) * k, lo, hi, sh, first, b0, v0);
      place(key, -M * k, lo, hi, sh, first, b1, v1);
      if (rows) {
        const uint32_t e = ev[n];
        if (e != kNoEvent) {
          place(key, 1, lo, hi, sh, first, b2, v2);
          place(e, -1, lo, hi, sh, first, b3, v3);
        }
      }
      // events of one node that share a bin (the usual case at the first digit) become one
      if (v1 != 0 && b1 == b0) { v0 += v1; v1 = 0; }
      if (v3 != 0 && b3 == b2) { v2 += v3; v3 = 0; }
    }
    wave_add(bins, b0, v0);
    wave_add(bins, b1, v1);
    if (rows) {
      wave_add(bins, b2, v2);
      wave_add(bins, b3, v3);
    }
  }
  __syncthreads();
  for (int t = threadIdx.x; t < kBins; t += 256) {
    const uint32_t v = bins[t];
    if (v) atomicAdd(&hist[t], v);
  }
}

// Pick of one digit, ONE workgroup of 1024 threads: suffix sums S_j = cost(hi) + sum_{i >= j} hist[i] = the cost at
// boundary j, the highest boundary j in [1, Q) with S_j > budget becomes lo and the next one hi (none: hi = boundary 1);
// the histogram is cleared for the next pass.  First pass only: S_0 = cost(tau_min) <= budget ends the descent with
// tau* = tau_min, and S_Q = cost(+inf) > budget fails the call.  After the last digit (sh = 0, hi = lo + 1) the result
// words tau*, cost(tau*) are stored.
__global__ __launch_bounds__(1024) void budget_pick_kernel(uint32_t* __restrict__ hist, uint32_t* __restrict__ state,
                                                           int sh, uint32_t budget) {
  __shared__ uint32_t suffix[kBins + 1];
  __shared__ uint32_t wave_tot[16];
  __shared__ int best;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (state[S_BAD]) {
    if (tid == 0) state[S_RESULT + 2] = kTauBadInput;
    return;
  }
  if (state[S_DONE] | state[S_FAIL]) return;
  const uint32_t lo = state[S_LO], hi = state[S_HI], cost_hi = state[S_COST_HI];
  const bool first = state[S_FIRST] != 0u;
  const int Q = (int)((hi >> sh) - (lo >> sh));
  // thread t owns bins j1 = kBins - 1 - 2 t and j0 = j1 - 1: ascending t = descending bins, so an inclusive scan over
  // the threads is a suffix sum over the bins
  const int j1 = kBins - 1 - 2 * tid, j0 = j1 - 1;
  const uint32_t h1 = hist[j1], h0 = hist[j0];
  hist[j1] = 0u;
  hist[j0] = 0u;
  uint32_t inc = h1 + h0;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t t = __shfl_up(inc, off, 64);
    if (lane >= off) inc += t;
  }
  if (lane == 63) wave_tot[wave] = inc;
  if (tid == 0) best = 0;
  __syncthreads();
  uint32_t base = cost_hi;
  for (int w = 0; w < wave; ++w) base += wave_tot[w];
  const uint32_t s0 = base + inc, s1 = s0 - h0;      // S_{j0}, S_{j1}
  suffix[j0] = s0;
  suffix[j1] = s1;
  if (tid == 0) suffix[kBins] = cost_hi;
  if (j1 >= 1 && j1 < Q && s1 > budget) atomicMax(&best, j1);
  else if (j0 >= 1 && j0 < Q && s0 > budget) atomicMax(&best, j0);
  __syncthreads();
  if (tid != 0) return;
  uint32_t* res = state + S_RESULT;
  if (first) {
    state[S_FIRST] = 0u;
    if (suffix[0] <= budget) {                      // the request fits: tau* = tau_min
      state[S_DONE] = 1u;
      res[2] = lo;
      res[3] = suffix[0];
      return;
    }
    if (suffix[Q] > budget) {                       // not even the coarsest cut does
      state[S_FAIL] = 1u;
      res[2] = kTauCapacity;
      res[3] = suffix[Q];
      return;
    }
  }
  const int j = best;
  const uint32_t nlo = j > 0 ? ((lo >> sh) + (uint32_t)j) << sh : lo;
  const uint32_t nhi = ((lo >> sh) + (uint32_t)j + 1u) << sh;
  state[S_LO] = nlo;
  state[S_HI] = nhi;
  state[S_COST_HI] = suffix[j + 1];
  if (sh == 0) {
    res[2] = nhi;
    res[3] = suffix[j + 1];
  }
}

// frustum_mark_kernel on the 4-byte sizes, tau* from device memory; a failed call marks nothing
__global__ __launch_bounds__(256) void budget_mark_kernel(const int32_t* __restrict__ nodes,
                                                          const uint32_t* __restrict__ sk, int N,
                                                          const uint32_t* __restrict__ state,
                                                          uint32_t* __restrict__ emit_cnt,
                                                          uint32_t* __restrict__ block_sums,
                                                          uint32_t* __restrict__ block_all,
                                                          unsigned long long* __restrict__ chain) {
  clear_scan_chain(chain, block_sums);
  const uint32_t tau_bits = state[S_RESULT + 2];
  const bool ok = tau_bits <= kInfBits;
  const int n = blockIdx.x * 256 + threadIdx.x;
  uint32_t cnt = 0, kept = 0;
  if (n < N && ok) {
    const int32_t* nd = nodes + (size_t)n * kNodeInts;
    const int par = nd[1];
    const uint32_t w = sk[n];
    // bit patterns of non-negative floats order as the floats do: s >= tau on the integers
    const bool coarse = (w & kKeyMask) >= tau_bits;
    const bool reached = coarse || par < 0 || (sk[par] & kKeyMask) >= tau_bits;
    cnt = cut_count(reached, coarse, nd);
    kept = (w >> 31) ? cnt : 0u;
  }
  if (n < N) emit_cnt[n] = kept;
  block_totals<2>({kept, cnt}, {block_sums, block_all});
}

__global__ __launch_bounds__(1024) void budget_scan_sums_kernel(uint32_t* __restrict__ sums,
                                                                const uint32_t* __restrict__ block_all, int n,
                                                                unsigned long long* __restrict__ chain, int c_off,
                                                                int chunks) {
  scan_sums_and_unculled_total(sums, block_all, n, chain, c_off, chunks);
}

// frustum_emit_kernel with the sizes from sk (the very bits node_size gave) and tau* from device memory; its first
// thread also puts the two totals beside tau* and the cost: the 16 bytes the host reads
__global__ __launch_bounds__(256) void budget_emit_kernel(const int32_t* __restrict__ nodes,
                                                          const uint32_t* __restrict__ sk,
                                                          const uint32_t* __restrict__ emit_cnt, int N,
                                                          uint32_t* __restrict__ state,
                                                          const uint32_t* __restrict__ block_sums,
                                                          int32_t* __restrict__ render_indices,
                                                          int32_t* __restrict__ parent_indices,
                                                          int32_t* __restrict__ node_indices,
                                                          float* __restrict__ weights,
                                                          int32_t* __restrict__ num_siblings, int capacity) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n == 0) {
    state[S_RESULT + 0] = block_sums[gridDim.x];
    state[S_RESULT + 1] = block_sums[gridDim.x + 1];
  }
  const uint32_t cnt = (n < N) ? emit_cnt[n] : 0u;
  const uint32_t off = block_exclusive_offset(cnt);
  if (cnt == 0) return;
  const float tau = __uint_as_float(state[S_RESULT + 2]);
  const int32_t* nd = nodes + (size_t)n * kNodeInts;
  const int start = nd[2];
  const int par = nd[1];
  int pstart = -1;
  float w = 1.0f;
  int kids = 1;
  if (par >= 0) {
    pstart = nodes[(size_t)par * kNodeInts + 2];
    w = interp_weight(__uint_as_float(sk[par] & kKeyMask), __uint_as_float(sk[n] & kKeyMask), tau);
    kids = nodes[(size_t)par * kNodeInts + 6];
  }
  write_entries<true>(block_sums[blockIdx.x] + off, cnt, capacity, n, start, pstart, render_indices, parent_indices,
                      node_indices, weights, w, num_siblings, kids);
}

struct BudgetTmp : SumsTmp {
  uint32_t* sk;          // [N] bits(s_n) | k_n << 31
  uint32_t* ev;          // [N] key of the parent's -1 event (cost = rows)
  uint32_t* emit_cnt;    // [N]
  uint32_t* hist;        // [kBins]
  uint32_t* state;       // [S_WORDS]
};

inline BudgetTmp carve_budget(Carver& c, int32_t N) {
  const size_t n = (size_t)(N > 0 ? N : 1);
  BudgetTmp t;
  t.sk = c.take<uint32_t>(n);
  t.ev = c.take<uint32_t>(n);
  t.emit_cnt = c.take<uint32_t>(n);
  static_cast<SumsTmp&>(t) = carve_sums(c, n, true);
  t.hist = c.take<uint32_t>(kBins);
  t.state = c.take<uint32_t>(S_WORDS);
  return t;
}

}  // namespace
}  // namespace hgs

using namespace hgs;

extern "C" {

size_t hgs_lod_cut_budget_tmp_bytes(int32_t N) {
  Carver c(nullptr);
  carve_budget(c, N);
  return c.bytes(kAlign);
}

int hgs_lod_cut_budget(const int32_t* nodes, const float* boxes, const float* bounds, int32_t N, float tau_min,
                       int32_t budget, int32_t cost_mode, const float viewpoint[3], const float planes[20],
                       float radius_scale, int32_t* render_indices, int32_t* parent_indices,
                       int32_t* nodes_for_render_indices, float* weights, int32_t* num_siblings, int32_t capacity,
                       void* tmp, int32_t* count_out_host, int32_t* unculled_out_host, float* tau_out_host,
                       int32_t* cost_out_host, hgs_stream_t stream, int device) {
  if (!count_out_host || !unculled_out_host || !tau_out_host || !cost_out_host) {
    set_error("lod_cut_budget: null result pointer");
    return HGS_ERR_INVALID;
  }
  *count_out_host = 0;
  *unculled_out_host = 0;
  *tau_out_host = tau_min;
  *cost_out_host = 0;
  if (N <= 0) { set_error("lod_cut_budget: N = %d", N); return HGS_ERR_INVALID; }
  if (!nodes || !boxes || !viewpoint || !render_indices || !parent_indices || !nodes_for_render_indices || !weights ||
      !num_siblings || !tmp) {
    set_error("lod_cut_budget: null argument");
    return HGS_ERR_INVALID;
  }
  if ((bounds == nullptr) != (planes == nullptr)) {
    set_error("lod_cut_budget: bounds and planes go together (both or neither)");
    return HGS_ERR_INVALID;
  }
  if (!(tau_min >= 0.0f)) { set_error("lod_cut_budget: tau_min = %g", (double)tau_min); return HGS_ERR_INVALID; }
  if (budget < 0) { set_error("lod_cut_budget: budget = %d", budget); return HGS_ERR_INVALID; }
  if (cost_mode != HGS_CUT_COST_ENTRIES && cost_mode != HGS_CUT_COST_ROWS) {
    set_error("lod_cut_budget: cost_mode = %d", cost_mode);
    return HGS_ERR_INVALID;
  }
  if (capacity < budget) {
    set_error("lod_cut_budget: the outputs hold %d entries, a budget of %d may need as many", capacity, budget);
    return HGS_ERR_INVALID;
  }
  HGS_HIP(hipSetDevice(device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  Carver c(tmp);
  const BudgetTmp t = carve_budget(c, N);
  const Vec3 vp = {viewpoint[0], viewpoint[1], viewpoint[2]};
  Frustum f;
  for (int k = 0; k < 5; ++k)
    f.p[k] = planes ? make_float4(planes[4 * k], planes[4 * k + 1], planes[4 * k + 2], planes[4 * k + 3])
                    : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  f.rs = radius_scale;
  const int nblk = (N + 255) / 256;
  const int rows = cost_mode == HGS_CUT_COST_ROWS ? 1 : 0;
  uint32_t tau_bits;
  const float tau_pos = tau_min + 0.0f;       // (-0 -> +0)
  memcpy(&tau_bits, &tau_pos, 4);
  // (hist and state are neighbours in the workspace: one memset)
  HGS_HIP(hipMemsetAsync(t.hist, 0, (size_t)(reinterpret_cast<char*>(t.state + S_WORDS) - reinterpret_cast<char*>(t.hist)), s));
  hipLaunchKernelGGL(budget_size_kernel, dim3(nblk), dim3(256), 0, s, nodes, boxes,
                     reinterpret_cast<const float4*>(bounds), N, vp, f, tau_bits, t.sk, t.state);
  HGS_LAUNCH_CHECK("budget_size", s, false);
  if (rows) {
    hipLaunchKernelGGL(budget_parent_kernel, dim3(nblk), dim3(256), 0, s, nodes, t.sk, N, t.ev, t.state + S_BAD);
    HGS_LAUNCH_CHECK("budget_parent", s, false);
  }
  const int hist_grid = nblk < kHistGrid ? nblk : kHistGrid;
  for (int sh = 20; sh >= 0; sh -= 10) {
    hipLaunchKernelGGL(budget_hist_kernel, dim3(hist_grid), dim3(256), 0, s, nodes, t.sk, t.ev, N, sh, rows, t.hist,
                       t.state);
    HGS_LAUNCH_CHECK("budget_hist", s, false);
    hipLaunchKernelGGL(budget_pick_kernel, dim3(1), dim3(1024), 0, s, t.hist, t.state, sh, (uint32_t)budget);
    HGS_LAUNCH_CHECK("budget_pick", s, false);
  }
  hipLaunchKernelGGL(budget_mark_kernel, dim3(nblk), dim3(256), 0, s, nodes, t.sk, N, t.state, t.emit_cnt,
                     t.block_sums, t.block_all, t.chain);
  HGS_LAUNCH_CHECK("budget_mark", s, false);
  const int rc = launch_scan_chunks(budget_scan_sums_kernel, "budget_scan_sums", nblk, s, t.block_sums, t.block_all,
                                    nblk, t.chain);
  if (rc != HGS_OK) return rc;
  hipLaunchKernelGGL(budget_emit_kernel, dim3(nblk), dim3(256), 0, s, nodes, t.sk, t.emit_cnt, N, t.state,
                     t.block_sums, render_indices, parent_indices, nodes_for_render_indices, weights, num_siblings,
                     capacity);
  HGS_LAUNCH_CHECK("budget_emit", s, false);
  uint32_t res[4] = {0, 0, 0, 0};             // kept, unculled, bits of tau*, cost(tau*): neighbours, one copy
  HGS_HIP(hipMemcpyAsync(res, t.state + S_RESULT, 16, hipMemcpyDeviceToHost, s));
  HGS_HIP(wait_stream(s));
  if (res[2] == kTauBadInput) {
    set_error("lod_cut_budget: a node record points outside the node list, or a node size is negative, NaN or larger "
              "than its parent's -- the boxes do not nest");
    return HGS_ERR_INVALID;
  }
  if (res[2] == kTauCapacity) {
    *cost_out_host = (int32_t)res[3];
    set_error("lod_cut_budget: the coarsest cut costs %u, more than the budget of %d", res[3], budget);
    return HGS_ERR_CAPACITY;
  }
  memcpy(tau_out_host, &res[2], 4);
  *count_out_host = (int32_t)res[0];
  *unculled_out_host = (int32_t)res[1];
  *cost_out_host = (int32_t)res[3];
  return HGS_OK;
}

}  // extern "C"
