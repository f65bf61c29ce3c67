// C ABI of libhgs.so (declared in include/hgs.h): argument validation, workspace
// carving, stage sequencing.  No torch types; the Python host (or any FFI) owns memory.
#include "common.h"

#include <pthread.h>
#include <sched.h>
#include <stdlib.h>
#include <time.h>
#include <string.h>

#include <atomic>
#include <cmath>
#include <mutex>
#include <vector>

namespace hgs {

// ---- optional per-stage timing (hipEvents on the caller's stream) ---------------
enum Stage { ST_PREPROCESS_FWD = 0, ST_SCAN, ST_DUPLICATE, ST_SORT, ST_RANGES, ST_SORT_DEPTH, ST_RENDER_FWD,
             ST_MEMSET_BWD, ST_RENDER_BWD, ST_PREPROCESS_BWD, ST_SH_BATCHED, ST_COUNT };
static const char* kStageNames[ST_COUNT] = {"preprocess_fwd", "scan", "duplicate_keys", "tile_sort", "tile_ranges",
                                            "tile_depth_sort", "render_fwd", "memset_bwd", "render_bwd",
                                            "preprocess_bwd", "sh_bwd_batched"};
struct Pending { int stage; hipEvent_t a, b; };
static uint32_t g_timing = 0;      // bit 0: every stage; bit (1 + stage): that stage only
static std::mutex g_tmu;
static std::vector<Pending> g_pending;
static std::vector<hipEvent_t> g_pool;
static double g_ms[ST_COUNT];
static uint32_t g_calls[ST_COUNT];

struct StageTimer {
  int stage; hipStream_t s; hipEvent_t a = nullptr, b = nullptr; bool on;
  StageTimer(int st, hipStream_t stream) : stage(st), s(stream), on((g_timing & (1u | (2u << st))) != 0) {
    if (!on) return;
    std::lock_guard<std::mutex> lk(g_tmu);
    for (hipEvent_t* e : {&a, &b}) {
      if (!g_pool.empty()) { *e = g_pool.back(); g_pool.pop_back(); }
      else if (hipEventCreate(e) != hipSuccess) { on = false; return; }
    }
    (void)hipEventRecord(a, s);
  }
  ~StageTimer() {
    if (!on) return;
    (void)hipEventRecord(b, s);
    std::lock_guard<std::mutex> lk(g_tmu);
    g_pending.push_back({stage, a, b});
  }
};
#define HGS_TIMED(stage, stream, expr) [&]() { hgs::StageTimer _t(stage, stream); return (expr); }()

static thread_local char g_err[512] = "";

// Per calling thread: 4 bytes of pinned, device-mapped host memory (the scan kernel stores the instance count there --
// no copy command in the stream; where the mapping is refused, a D2H copy into it: a copy into pageable memory would
// block the host until it has run, which would defeat enqueue-ahead in hgs_raster_fwd) and ONE reusable event per device.  Both are released by a
// pthread key destructor when the thread ends (autograd worker threads come and go); a thread that is still alive
// at process exit leaves them to the driver's teardown, which is the only safe order.
constexpr int kMaxDevices = 16;
struct ThreadHost {
  uint32_t* pinned_L = nullptr;
  hipEvent_t ev[kMaxDevices] = {};     // one per device: an event is recorded on streams of the device it was created on
};
static pthread_key_t g_host_key;
static pthread_once_t g_host_once = PTHREAD_ONCE_INIT;
static void thread_host_free(void* p) {
  ThreadHost* h = static_cast<ThreadHost*>(p);
  if (!h) return;
  for (int i = 0; i < kMaxDevices; ++i)
    if (h->ev[i]) (void)hipEventDestroy(h->ev[i]);
  if (h->pinned_L) (void)hipHostFree(h->pinned_L);
  delete h;
}
static void thread_host_key_init() { (void)pthread_key_create(&g_host_key, thread_host_free); }
// call after hipSetDevice(device): the event of that device is created on first use
static ThreadHost* thread_host(int device) {
  if (device < 0 || device >= kMaxDevices) return nullptr;
  (void)pthread_once(&g_host_once, thread_host_key_init);
  ThreadHost* h = static_cast<ThreadHost*>(pthread_getspecific(g_host_key));
  if (!h) {
    h = new ThreadHost();
    if (hipHostMalloc(reinterpret_cast<void**>(&h->pinned_L), sizeof(uint32_t), hipHostMallocPortable | hipHostMallocMapped) != hipSuccess) {
      thread_host_free(h);
      return nullptr;
    }
    (void)pthread_setspecific(g_host_key, h);
  }
  if (!h->ev[device] && hipEventCreateWithFlags(&h->ev[device], hipEventDisableTiming) != hipSuccess) {
    h->ev[device] = nullptr;
    return nullptr;
  }
  return h;
}

static bool blocking_waits() {
  static const bool b = getenv("HGS_BLOCKING_WAIT") != nullptr;
  return b;
}
static inline void cpu_relax() {
#if defined(__x86_64__) || defined(__i386__)
  __builtin_ia32_pause();
#elif defined(__aarch64__) || defined(__arm__)
  __asm__ __volatile__("yield");
#else
  sched_yield();
#endif
}
template <typename Query>
static bool poll_done(Query query, hipError_t* result) {
  if (blocking_waits()) return false;
  timespec t0;
  clock_gettime(CLOCK_MONOTONIC, &t0);
  for (unsigned i = 0;; ++i) {
    const hipError_t q = query();
    if (q != hipErrorNotReady) { *result = q; return true; }
    (void)hipGetLastError();                       // "not ready" is not an error to keep
    cpu_relax();
    if ((i & 255u) == 255u) {
      timespec t;
      clock_gettime(CLOCK_MONOTONIC, &t);
      if ((t.tv_sec - t0.tv_sec) * 1000000000LL + (t.tv_nsec - t0.tv_nsec) > 200000000LL) return false;
    }
  }
}
hipError_t wait_stream(hipStream_t s) {
  hipError_t r;
  if (poll_done([&] { return hipStreamQuery(s); }, &r)) return r;
  return hipStreamSynchronize(s);
}
hipError_t wait_event(hipEvent_t e) {
  hipError_t r;
  if (poll_done([&] { return hipEventQuery(e); }, &r)) return r;
  return hipEventSynchronize(e);
}

// 1024-thread workgroups of the chained scan that are certainly resident together = compute units of the device -- as far
// as this process can tell: the attribute does not see a CU mask (HSA_CU_MASK, ROC_GLOBAL_CU_MASK), so with one of them
// in the environment the answer is 1 (the scans then run one chunk per launch: slow and correct).  The scan launch itself is the fallback route since round 5 (preprocess.hip: superblock totals).
int scan_resident_workgroups() {
  static std::atomic<int> cus[kMaxDevices];
  static const bool masked = getenv("HSA_CU_MASK") || getenv("ROC_GLOBAL_CU_MASK") || getenv("HSA_CU_MASK_SKIP_INIT");
  if (masked) return 1;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return 1;
  int n = cus[dev].load(std::memory_order_relaxed);
  if (n == 0) {
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1) n = 1;
    cus[dev].store(n, std::memory_order_relaxed);
  }
  return n;
}
bool scan_split_forced() {
  static const bool b = getenv("HGS_SCAN_SPLIT") != nullptr;
  return b;
}

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

// The four raster workspaces: layout() is the one text of each (common.h: carve_from() and bytes() run it).
GeomWs GeomWs::layout(Carver& c, int32_t P) {
  const size_t p = (size_t)(P > 0 ? P : 1);
  const size_t nblk = (p + kPreBlock - 1) / kPreBlock;
  const size_t jac_rows = (p + 63) / 64 * 64;   // K1's H48 route stores the Jacobians of whole 64-row waves
  GeomWs g;
  g.records = c.take<float>(p * kRecFloats);
  g.depths = c.take<float>(p);
  g.rects = c.take<uint32_t>(p * 2);
  g.tiles_touched = c.take<uint32_t>(p);
  g.offsets = c.take<uint32_t>(p);
  g.flags = c.take<uint32_t>(p);
  g.block_sums = c.take<uint32_t>(nblk + 1);
  g.block_band = c.take<uint32_t>((nblk + 1) * kBands);
  g.shjac = c.take<float>(jac_rows * kJacStride);
  g.scan_chain = c.take<unsigned long long>((size_t)(1 + kBands) * scan_chunks(nblk));
  return g;
}

BinWs BinWs::layout(Carver& c, uint32_t L, int32_t T) {
  const size_t l = L ? L : 1, tmp_sort = sort_tmp_bytes((uint32_t)l), tmp_bin = tile_bin_tmp_bytes(L, T);
  BinWs b;
  b.keys_in = c.take<uint32_t>(l);
  b.vals_in = c.take<uint32_t>(l);
  b.keys_out = c.take<uint32_t>(l);
  b.vals_out = c.take<uint32_t>(l);
  b.ranges = c.take<uint32_t>((size_t)T * 2);
  b.big_tiles = c.take<uint32_t>((size_t)T * 3 + 3);
  b.tile_order = c.take<uint32_t>((size_t)T + 8);    // 8 * ceil(T / 8) entries
  b.sort_tmp = c.take<char>(tmp_sort > tmp_bin ? tmp_sort : tmp_bin);   // nested: either figure has its own slack
  return b;
}

// (a braced list is evaluated left to right)
ImgWs ImgWs::layout(Carver& c, int32_t W, int32_t H) { return {c.take<float>((size_t)W * H), c.take<uint32_t>((size_t)W * H)}; }

BwdWs BwdWs::layout(Carver& c, uint32_t L, int32_t P) {
  const size_t l = L ? L : 1, p = (size_t)(P > 0 ? P : 1);
  BwdWs w;
  w.inst_grads = c.take<float>(l * kInstStride);
  w.drgb = c.take<float>(p * 3);
  w.dmean_rows = c.take<float>(p * 3);
  w.lod_flag = c.take<uint32_t>(kAlign / sizeof(uint32_t));   // one block: the flag word and the worklist counter
  w.work_counter = w.lod_flag ? w.lod_flag + 16 : nullptr;
  w.work = c.take<uint2>(l / kK8LongRun + 2);
  return w;
}

static int validate(const hgs_raster_args* a) {
  if (!a) { set_error("null args"); return HGS_ERR_INVALID; }
  if (a->P < 0 || a->width <= 0 || a->height <= 0) { set_error("bad sizes P=%d W=%d H=%d", a->P, a->width, a->height); return HGS_ERR_INVALID; }
  if (grid_x(a->width) > 1023 || grid_y(a->height) > 1023) { set_error("image larger than 16368 px per side is not supported"); return HGS_ERR_INVALID; }
  if (!a->bg || !a->viewmatrix || !a->projmatrix || !a->campos) { set_error("bg/viewmatrix/projmatrix/campos must be device pointers"); return HGS_ERR_INVALID; }
  // half-precision attribute rows (lod_half_rows): one forward-only instantiation of K1's in-kernel LOD route reads them
  if (a->lod_half_rows != 0 && a->lod_half_rows != 1) { set_error("lod_half_rows = %d: 0 (float32 rows) or 1 (half rows)", a->lod_half_rows); return HGS_ERR_INVALID; }
  if (a->lod_half_rows) {
    if (!a->lod_render_indices) { set_error("lod_half_rows needs lod_render_indices: half rows are read by the in-kernel LOD interpolation only"); return HGS_ERR_INVALID; }
    if (a->prepare_backward) { set_error("lod_half_rows is forward only: prepare_backward must be 0"); return HGS_ERR_INVALID; }
    if (a->shs_rest || a->activations || a->colors_precomp || a->cov3D_precomp) { set_error("lod_half_rows takes shs, scales and rotations as halves: no shs_rest, activations, colors_precomp or cov3D_precomp"); return HGS_ERR_INVALID; }
  }
  if (a->P > 0) {
    if (!a->means3D || !a->opacities) { set_error("means3D/opacities missing"); return HGS_ERR_INVALID; }
    if ((a->shs != nullptr) == (a->colors_precomp != nullptr)) { set_error("provide exactly one of shs / colors_precomp"); return HGS_ERR_INVALID; }
    const bool sr = a->scales && a->rotations;
    if (sr == (a->cov3D_precomp != nullptr) || ((a->scales != nullptr) != (a->rotations != nullptr))) {
      set_error("provide exactly one of (scales, rotations) / cov3D_precomp");
      return HGS_ERR_INVALID;
    }
    if (a->shs) {
      if (a->sh_degree < 0 || a->sh_degree > 3) { set_error("sh_degree %d not in 0..3", a->sh_degree); return HGS_ERR_INVALID; }
      if (a->M < (a->sh_degree + 1) * (a->sh_degree + 1) || a->M > 16) { set_error("M=%d incompatible with sh_degree=%d (max 16 coefficients)", a->M, a->sh_degree); return HGS_ERR_INVALID; }
    }
    // the SH blocks and the quaternions are moved with 16-byte accesses
    if (((uintptr_t)a->shs | (uintptr_t)a->shs_rest | (uintptr_t)a->rotations) & 15u) { set_error("shs / shs_rest / rotations must be 16-byte aligned"); return HGS_ERR_INVALID; }
    if (a->defer_sh_bwd && a->shs_rest) { set_error("defer_sh_bwd is not available with split SH storage (shs_rest)"); return HGS_ERR_INVALID; }
    if (a->shs_rest && (!a->shs || a->M < 2)) { set_error("shs_rest needs shs (features_dc) and M >= 2"); return HGS_ERR_INVALID; }
    if ((a->activations & HGS_ACT_OPACITY_SIGMOID) && (a->activations & HGS_ACT_OPACITY_ABS)) { set_error("choose one opacity activation"); return HGS_ERR_INVALID; }
    if ((a->activations & (HGS_ACT_SCALE_EXP | HGS_ACT_ROT_NORMALIZE)) && a->cov3D_precomp) { set_error("scale / rotation activations need scales and rotations"); return HGS_ERR_INVALID; }
    if ((a->interpolation_weights != nullptr) != (a->num_node_kids != nullptr)) { set_error("interpolation_weights and num_node_kids must be given together"); return HGS_ERR_INVALID; }
    if ((a->lod_render_indices != nullptr) != (a->lod_parent_indices != nullptr)) { set_error("lod_render_indices and lod_parent_indices must be given together"); return HGS_ERR_INVALID; }
    if (a->lod_render_indices) {
      if (!a->shs || a->shs_rest || !a->scales || !a->rotations || a->activations || !a->interpolation_weights) { set_error("in-kernel LOD interpolation needs shs, scales, rotations, interpolation_weights / num_node_kids and no activations"); return HGS_ERR_INVALID; }
      if (a->lod_n < 0 || a->lod_n > a->P || a->lod_rows < a->P - a->lod_n) { set_error("bad lod_n / lod_rows (P=%d lod_n=%d lod_rows=%d)", a->P, a->lod_n, a->lod_rows); return HGS_ERR_INVALID; }
      if (a->defer_sh_bwd || a->accumulate_grads) { set_error("defer_sh_bwd / accumulate_grads are not available with in-kernel LOD interpolation"); return HGS_ERR_INVALID; }
    }
  }
  return HGS_OK;
}

}  // namespace hgs

using namespace hgs;

extern "C" {

int hgs_abi_version(void) { return HGS_ABI_VERSION; }
const char* hgs_last_error(void) { return g_err; }
int hgs_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return -1;
  return n;
}

int hgs_raster_ws_sizes(int32_t P, int32_t width, int32_t height, uint32_t L, size_t* geom_bytes,
                        size_t* bin_bytes, size_t* img_bytes, size_t* bwd_bytes) {
  if (P < 0 || width <= 0 || height <= 0) { set_error("bad sizes"); return HGS_ERR_INVALID; }
  const int T = grid_x(width) * grid_y(height);
  if (geom_bytes) *geom_bytes = GeomWs::bytes(P);
  if (bin_bytes) *bin_bytes = BinWs::bytes(L, T);
  if (img_bytes) *img_bytes = ImgWs::bytes(width, height);
  if (bwd_bytes) *bwd_bytes = BwdWs::bytes(L, P);
  return HGS_OK;
}

int hgs_raster_fwd_stage1(const hgs_raster_args* a, void* geom_ws, int32_t* radii, uint32_t* L_out_host,
                          hgs_stream_t stream, int device) {
  int rc = validate(a);
  if (rc) return rc;
  if (!geom_ws || !L_out_host || (a->P > 0 && !radii)) { set_error("null workspace/output"); return HGS_ERR_INVALID; }
  HGS_HIP(hipSetDevice(device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const GeomWs g = GeomWs::carve_from(geom_ws, a->P);
  *L_out_host = 0;
  if (a->P == 0) return HGS_OK;
  if ((rc = HGS_TIMED(ST_PREPROCESS_FWD, s, launch_preprocess_fwd(*a, g, radii, s)))) return rc;
  if ((rc = HGS_TIMED(ST_SCAN, s, launch_scan_block_sums(g, a->P, s, a->debug)))) return rc;
  const int nblk = (a->P + kPreBlock - 1) / kPreBlock;
  HGS_HIP(hipMemcpyAsync(L_out_host, g.block_sums + nblk, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  HGS_HIP(wait_stream(s));
  return HGS_OK;
}

// Stage-2 launches.  L is exact when L_dev == nullptr; otherwise it is a capacity and the kernels read the
// actual instance count from device memory.
// super != nullptr (single-call forward only): K1 left raw workgroup sums + superblock totals, K3 finishes the scans and
// is the kernel that produces the instance count -- into *mirror (mapped host word) or, without a mapping, by a copy
// into `stage` -- and `ev` is recorded right behind it.
static int enqueue_stage2(const hgs_raster_args* a, const GeomWs& g, const BinWs& b, const ImgWs& im, uint32_t L,
                          const uint32_t* L_dev, int T, float* out_color, float* out_invdepth, hipStream_t s,
                          uint32_t* super = nullptr, uint32_t* mirror = nullptr, uint32_t* stage = nullptr,
                          hipEvent_t ev = nullptr) {
  int rc;
  const bool bin = L > 0 && tile_bin_supported(T);
  if ((rc = HGS_TIMED(ST_DUPLICATE, s, launch_duplicate_tiles(*a, g, b, L, bin, s, super, mirror)))) return rc;   // also zeroes b.ranges
  if (super) {
    if (!mirror) HGS_HIP(hipMemcpyAsync(stage, L_dev, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HGS_HIP(hipEventRecord(ev, s));
  }
  if (bin) {            // counting pass + scatter pass per tile band; writes the tile ranges too
    const int nblk = (a->P + kPreBlock - 1) / kPreBlock;
    if ((rc = HGS_TIMED(ST_SORT, s, launch_tile_bin(b.keys_in, b.vals_in, b.vals_out, b.sort_tmp, L, g.block_band, nblk, T, b.ranges, b.big_tiles, b.tile_order, super, s, a->debug)))) return rc;
  } else {              // very large tile grids: stable radix sort by tile id, then ranges off the sorted ids
    if (L > 0) {
      if ((rc = HGS_TIMED(ST_SORT, s, sort_pairs32(b.keys_in, b.vals_in, b.keys_out, b.vals_out, b.sort_tmp, L, L_dev, tile_bits(T), s, a->debug)))) return rc;
    }
    if ((rc = HGS_TIMED(ST_RANGES, s, launch_tile_ranges(b, L, L_dev, T, s, a->debug)))) return rc;
  }
  // (the sorted tile-id column is introspection: the binning path only writes it for a debug forward)
  if ((rc = HGS_TIMED(ST_SORT_DEPTH, s, launch_tile_depth_sort(*a, g, b, L, T, bin && a->debug, s)))) return rc;
  if (!bin && (rc = launch_tile_order(b, T, s, a->debug))) return rc;   // (the binning path orders inside its scatter launch)
  return HGS_TIMED(ST_RENDER_FWD, s, launch_render_fwd(*a, g, b, im, out_color, out_invdepth, s));
}

int hgs_raster_fwd_stage2(const hgs_raster_args* a, void* geom_ws, void* bin_ws, void* img_ws, uint32_t L,
                          float* out_color, float* out_invdepth, hgs_stream_t stream, int device) {
  int rc = validate(a);
  if (rc) return rc;
  if (!geom_ws || !bin_ws || !img_ws || !out_color) { set_error("null workspace/output"); return HGS_ERR_INVALID; }
  HGS_HIP(hipSetDevice(device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int T = grid_x(a->width) * grid_y(a->height);
  const GeomWs g = GeomWs::carve_from(geom_ws, a->P);
  const BinWs b = BinWs::carve_from(bin_ws, L, T);
  const ImgWs im = ImgWs::carve_from(img_ws, a->width, a->height);
  return enqueue_stage2(a, g, b, im, L, nullptr, T, out_color, out_invdepth, s);
}

int hgs_raster_fwd(const hgs_raster_args* a, void* geom_ws, void* bin_ws, void* img_ws, uint32_t L_cap,
                   int32_t* radii, float* out_color, float* out_invdepth, uint32_t* L_out_host,
                   hgs_stream_t stream, int device) {
  int rc = validate(a);
  if (rc) return rc;
  if (!geom_ws || !bin_ws || !img_ws || !out_color || !L_out_host || (a->P > 0 && !radii)) {
    set_error("null workspace/output");
    return HGS_ERR_INVALID;
  }
  HGS_HIP(hipSetDevice(device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int T = grid_x(a->width) * grid_y(a->height);
  const GeomWs g = GeomWs::carve_from(geom_ws, a->P);
  const BinWs b = BinWs::carve_from(bin_ws, L_cap, T);
  const ImgWs im = ImgWs::carve_from(img_ws, a->width, a->height);
  *L_out_host = 0;
  if (a->P == 0) return enqueue_stage2(a, g, b, im, 0, nullptr, T, out_color, out_invdepth, s);
  ThreadHost* th = thread_host(device);
  if (!th) { set_error("cannot allocate pinned host memory / event (device %d)", device); return HGS_ERR_NOMEM; }
  hipEvent_t ev = th->ev[device];
  uint32_t* stage = th->pinned_L;
  // the scan kernel stores the count into the mapped host word itself (visible to the host once the event after the
  // kernel has fired: a kernel's writes are released to system scope when it ends)
  static const bool by_copy = getenv("HGS_COUNT_BY_COPY") != nullptr;     // diagnostic: the copy command instead
  void* mirror = nullptr;
  if (by_copy || hipHostGetDevicePointer(&mirror, stage, 0) != hipSuccess) { (void)hipGetLastError(); mirror = nullptr; }
  // No scan launch on the usual path: K1 adds its workgroup sums to zeroed superblock totals and K3 finishes the scans
  // (preprocess.hip, binning.hip).  The scan launch remains for tile grids that take the radix path, for more than
  // kSuper * kMaxSuper workgroups (16.7 M rows) and when no zeroed block is to be had (HGS_SCAN_LAUNCH=1 forces it).
  const int nblk = (a->P + kPreBlock - 1) / kPreBlock;
  uint32_t* super = nullptr;
  if (L_cap > 0 && tile_bin_supported(T) && nblk <= kSuper * kMaxSuper) super = super_block_acquire(s);
  if ((rc = HGS_TIMED(ST_PREPROCESS_FWD, s, launch_preprocess_fwd(*a, g, radii, s, super, super ? k3_heavy_threshold(L_cap, a->P) : 0u)))) {
    if (super) super_block_mark_dirty(super);
    return rc;
  }
  const uint32_t* L_dev = g.block_sums + nblk;
  hipError_t e = hipSuccess;
  if (!super) {
    if ((rc = HGS_TIMED(ST_SCAN, s, launch_scan_block_sums(g, a->P, s, a->debug, static_cast<uint32_t*>(mirror))))) return rc;
    if (!mirror) HGS_HIP(hipMemcpyAsync(stage, L_dev, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    e = hipEventRecord(ev, s);
  }
  // everything else is enqueued before the host looks at L: the GPU never waits for the host
  if (e == hipSuccess) rc = enqueue_stage2(a, g, b, im, L_cap, L_dev, T, out_color, out_invdepth, s, super,
                                           static_cast<uint32_t*>(mirror), stage, ev);
  if (rc || e != hipSuccess) {
    // the superblock totals may not have been consumed and cleared: zero them before the next use
    if (super) super_block_mark_dirty(super);
    if (rc) return rc;
  }
  if (e == hipSuccess) e = wait_event(ev);
  if (e != hipSuccess) { set_error("hgs_raster_fwd: %s", hipGetErrorString(e)); return HGS_ERR_HIP; }
  *L_out_host = *stage;
  if (rc) return rc;
  if (*L_out_host > L_cap) {
    if (super) {
      // the caller finishes on hgs_raster_fwd_stage2 over THIS geometry workspace, whose K3 expects the workgroup sums
      // scanned: scan the raw sums now (the superblock totals are consumed and cleared; this path is the rare one)
      HGS_HIP(hipMemsetAsync(g.scan_chain, 0, (size_t)(1 + kBands) * scan_chunks(nblk) * sizeof(unsigned long long), s));
      if ((rc = launch_scan_block_sums(g, a->P, s, a->debug, nullptr))) return rc;
    }
    set_error("instance count %u exceeds the capacity %u given to hgs_raster_fwd", *L_out_host, L_cap);
    return HGS_ERR_CAPACITY;
  }
  return HGS_OK;
}

int hgs_release_device_state(int device) { return super_block_release(device); }

int hgs_raster_bwd(const hgs_raster_args* a, const void* geom_ws, const void* bin_ws, const void* img_ws,
                   void* bwd_ws, uint32_t L, const float* out_color, const float* out_invdepth,
                   const float* dL_dcolor, const float* dL_dinvdepth, const hgs_raster_grads* grads,
                   hgs_stream_t stream, int device) {
  if (a && a->lod_half_rows != 0) { set_error("hgs_raster_bwd: lod_half_rows is forward only (there is no backward through half rows)"); return HGS_ERR_INVALID; }
  int rc = validate(a);
  if (rc) return rc;
  if (!geom_ws || !bin_ws || !img_ws || !bwd_ws || !out_color || !dL_dcolor || !grads) { set_error("null workspace/input"); return HGS_ERR_INVALID; }
  if (a->lod_render_indices && !a->prepare_backward) { set_error("the backward of an in-kernel LOD interpolation needs prepare_backward = 1 in the forward and the backward call"); return HGS_ERR_INVALID; }
  if (a->lod_scatter && (!a->lod_render_indices || ((a->M * 3) & 3) != 0 || a->accumulate_grads || a->defer_sh_bwd)) { set_error("lod_scatter needs in-kernel LOD interpolation, 3M %% 4 == 0, no accumulation and no deferred SH backward"); return HGS_ERR_INVALID; }
  if (a->P > 0) {
    if (!grads->dL_dmeans3D || !grads->dL_dmeans2D || !grads->dL_dopacity) { set_error("missing gradient outputs"); return HGS_ERR_INVALID; }
    if ((a->shs && !grads->dL_dshs) || (a->shs_rest && !grads->dL_dshs_rest) || (a->colors_precomp && !grads->dL_dcolors) ||
        (a->scales && (!grads->dL_dscales || !grads->dL_drotations)) || (a->cov3D_precomp && !grads->dL_dcov3D)) {
      set_error("gradient outputs do not match the inputs that were provided");
      return HGS_ERR_INVALID;
    }
  }
  HGS_HIP(hipSetDevice(device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (a->P == 0) return HGS_OK;
  const int T = grid_x(a->width) * grid_y(a->height);
  const GeomWs g = GeomWs::carve_from(const_cast<void*>(geom_ws), a->P);
  const BinWs b = BinWs::carve_from(const_cast<void*>(bin_ws), L, T);
  const ImgWs im = ImgWs::carve_from(const_cast<void*>(img_ws), a->width, a->height);
  BwdWs w = BwdWs::carve_from(bwd_ws, L, a->P);
  if (L > 0) {     // (the instance scratch needs no clearing: K7 writes every record, sums or zeros)
    if ((rc = HGS_TIMED(ST_RENDER_BWD, s, launch_render_bwd(*a, g, b, im, out_color, out_invdepth, dL_dcolor, dL_dinvdepth, w.inst_grads, s)))) return rc;
  }
  hgs_raster_grads gr = *grads;
  if (!a->shs) gr.dL_dshs = nullptr;
  if (!a->shs_rest) gr.dL_dshs_rest = nullptr;
  if (!a->colors_precomp) gr.dL_dcolors = nullptr;
  if (!a->scales) { gr.dL_dscales = nullptr; gr.dL_drotations = nullptr; }
  if (!a->cov3D_precomp) gr.dL_dcov3D = nullptr;
  if (!(a->lod_render_indices && a->lod_scatter)) w.lod_flag = nullptr;
  if (w.lod_flag) {
    HGS_HIP(hipMemsetAsync(w.lod_flag, 0, sizeof(uint32_t), s));
    if ((rc = launch_lod_monotone(a->lod_parent_indices, a->lod_n, w.lod_flag, s))) return rc;
  }
  return HGS_TIMED(ST_PREPROCESS_BWD, s, launch_preprocess_bwd(*a, g, w, gr, L, s));
}

// What the four calls that read a finished forward share (hgs_raster_contrib / _attribute / _pixels / _values), in two halves
// because a call's own argument checks stand between them in the documented order of refusals.
// First half: the argument check and the lod_per_pixel refusal.
static int check_forward_read(const char* fn, const char* follows, const hgs_raster_args* a) {
  const int rc = validate(a);
  if (rc) return rc;
  if (a->lod_per_pixel != 0) { set_error("%s: lod_per_pixel = %d is not built (the %s the per-Gaussian remap only)", fn, a->lod_per_pixel, follows); return HGS_ERR_INVALID; }
  return HGS_OK;
}

// Second half: the slot-count checks, the null-workspace check, the device and the carving of the forward's workspaces.
// `arrays`: n_slots is the length of per-slot output arrays (the identity map then needs P of them); otherwise it only
// bounds slot_of_row.  An empty forward (P == 0 or L == 0) has nothing carved, and only a call that still has planes to
// fill (`runs_empty`) selects the device for it; the others are done (f.empty, HGS_OK).
struct ForwardRead {
  GeomWs g{};
  BinWs b{};
  hipStream_t s = nullptr;
  bool empty = true;
};
static int open_forward_read(const char* fn, const char* ws_names, const hgs_raster_args* a, const void* geom_ws,
                             const void* bin_ws, const void* img_ws, bool tmp_missing, uint32_t L,
                             const int32_t* slot_of_row, int64_t n_slots, bool arrays, bool runs_empty,
                             hgs_stream_t stream, int device, ForwardRead& f) {
  if (arrays) {
    if (n_slots < 1) { set_error("%s: n_slots = %lld, need >= 1", fn, (long long)n_slots); return HGS_ERR_INVALID; }
    if (!slot_of_row && n_slots < a->P) { set_error("%s: n_slots = %lld < P = %d without slot_of_row (the identity map)", fn, (long long)n_slots, a->P); return HGS_ERR_INVALID; }
  } else if (slot_of_row && n_slots < 1) {
    set_error("%s: n_slots = %lld with slot_of_row, need >= 1", fn, (long long)n_slots);
    return HGS_ERR_INVALID;
  }
  f.empty = a->P == 0 || L == 0;
  if (f.empty && !runs_empty) return HGS_OK;
  if (!f.empty && (!geom_ws || !bin_ws || !img_ws || tmp_missing)) { set_error("%s: null workspace (%s)", fn, ws_names); return HGS_ERR_INVALID; }
  HGS_HIP(hipSetDevice(device));
  f.s = static_cast<hipStream_t>(stream);
  if (!f.empty) {
    f.g = GeomWs::carve_from(const_cast<void*>(geom_ws), a->P);
    f.b = BinWs::carve_from(const_cast<void*>(bin_ws), L, grid_x(a->width) * grid_y(a->height));
  }
  return HGS_OK;
}

size_t hgs_raster_contrib_tmp_bytes(uint32_t L) { return ContribWs::bytes(L); }

int hgs_raster_contrib(const hgs_raster_args* a, const void* geom_ws, const void* bin_ws, const void* img_ws,
                       uint32_t L, const uint8_t* pixel_mask, const int32_t* slot_of_row, int64_t n_slots,
                       float* wmax, double* wsum, int64_t* count, void* tmp, hgs_stream_t stream, int device) {
  int rc = check_forward_read("hgs_raster_contrib", "statistics follow", a);
  if (rc) return rc;
  if (!wmax || !wsum || !count) { set_error("hgs_raster_contrib: null output (wmax / wsum / count)"); return HGS_ERR_INVALID; }
  ForwardRead f;
  rc = open_forward_read("hgs_raster_contrib", "geom / bin / img / tmp", a, geom_ws, bin_ws, img_ws, !tmp, L, slot_of_row,
                         n_slots, true, false, stream, device, f);
  if (rc || f.empty) return rc;
  return launch_raster_contrib(*a, f.g, f.b, ContribWs::carve_from(tmp, L), L, pixel_mask, slot_of_row, n_slots, wmax,
                               wsum, count, f.s);
}

size_t hgs_raster_attribute_tmp_bytes(uint32_t L) { return AttributeWs::bytes(L); }

int hgs_raster_attribute(const hgs_raster_args* a, const void* geom_ws, const void* bin_ws, const void* img_ws,
                         uint32_t L, const float* image, int32_t channels, const uint8_t* pixel_mask,
                         const int32_t* slot_of_row, int64_t n_slots, double* out, double* wsum, void* tmp,
                         hgs_stream_t stream, int device) {
  int rc = check_forward_read("hgs_raster_attribute", "weights follow", a);
  if (rc) return rc;
  if (channels < 1 || channels > 3) { set_error("hgs_raster_attribute: channels = %d, need 1..3", channels); return HGS_ERR_INVALID; }
  if (!image) { set_error("hgs_raster_attribute: null image"); return HGS_ERR_INVALID; }
  if (!out) { set_error("hgs_raster_attribute: null output (out)"); return HGS_ERR_INVALID; }
  ForwardRead f;
  rc = open_forward_read("hgs_raster_attribute", "geom / bin / img / tmp", a, geom_ws, bin_ws, img_ws, !tmp, L,
                         slot_of_row, n_slots, true, false, stream, device, f);
  if (rc || f.empty) return rc;
  return launch_raster_attribute(*a, f.g, f.b, AttributeWs::carve_from(tmp, L), L, image, channels, pixel_mask,
                                 slot_of_row, n_slots, out, wsum, f.s);
}

int hgs_raster_pixels(const hgs_raster_args* a, const void* geom_ws, const void* bin_ws, const void* img_ws, uint32_t L,
                      const int32_t* slot_of_row, int64_t n_slots, const hgs_raster_pixel_planes* out,
                      hgs_stream_t stream, int device) {
  int rc = check_forward_read("hgs_raster_pixels", "readout follows", a);
  if (rc) return rc;
  if (!out || (!out->alpha && !out->count && !out->front && !out->back && !out->heaviest && !out->wmax && !out->median && !out->median_depth)) {
    set_error("hgs_raster_pixels: null planes (at least one of alpha / count / front / back / heaviest / wmax / median / median_depth is needed)");
    return HGS_ERR_INVALID;
  }
  ForwardRead f;
  rc = open_forward_read("hgs_raster_pixels", "geom / bin / img", a, geom_ws, bin_ws, img_ws, false, L, slot_of_row,
                         n_slots, false, true, stream, device, f);
  if (rc) return rc;
  return launch_raster_pixels(*a, f.g, f.b, f.empty, slot_of_row, n_slots, *out, f.s);    // empty: nothing carved
}

int hgs_raster_values(const hgs_raster_args* a, const void* geom_ws, const void* bin_ws, const void* img_ws, uint32_t L,
                      const float* values, int64_t value_stride, int channels, const int32_t* slot_of_row,
                      int64_t n_slots, const float* background, float* out, float* wsum, hgs_stream_t stream,
                      int device) {
  int rc = check_forward_read("hgs_raster_values", "blend follows", a);
  if (rc) return rc;
  if (channels < 1 || channels > 4) { set_error("hgs_raster_values: channels = %d, need 1..4", channels); return HGS_ERR_INVALID; }
  if (value_stride < channels) { set_error("hgs_raster_values: value_stride = %lld < channels = %d", (long long)value_stride, channels); return HGS_ERR_INVALID; }
  if (!values) { set_error("hgs_raster_values: null values"); return HGS_ERR_INVALID; }
  if (!out) { set_error("hgs_raster_values: null output (out)"); return HGS_ERR_INVALID; }
  ForwardRead f;
  rc = open_forward_read("hgs_raster_values", "geom / bin / img", a, geom_ws, bin_ws, img_ws, false, L, slot_of_row,
                         n_slots, true, true, stream, device, f);
  if (rc) return rc;
  return launch_raster_values(*a, f.g, f.b, f.empty, values, value_stride, channels, slot_of_row, n_slots, background,
                              out, wsum, f.s);                                            // empty: nothing carved
}

int hgs_raster_sh_bwd_batched(const hgs_sh_bwd_view* views, int32_t n_views, int32_t P, int32_t M, int32_t sh_degree,
                              const float* means3D, const float* shs, float* dL_dshs, float* dL_dmeans3D,
                              int32_t accumulate, hgs_stream_t stream, int device) {
  if (n_views <= 0 || P <= 0) return HGS_OK;
  if (!views || n_views > HGS_MAX_DEFERRED_VIEWS) { set_error("1..%d deferred views per call", HGS_MAX_DEFERRED_VIEWS); return HGS_ERR_INVALID; }
  if (!means3D || !shs || !dL_dshs || !dL_dmeans3D) { set_error("null argument"); return HGS_ERR_INVALID; }
  if (sh_degree < 0 || sh_degree > 3 || M < (sh_degree + 1) * (sh_degree + 1) || M > 16) { set_error("M=%d incompatible with sh_degree=%d", M, sh_degree); return HGS_ERR_INVALID; }
  if (((uintptr_t)shs | (uintptr_t)dL_dshs) & 15u) { set_error("shs / dL_dshs must be 16-byte aligned"); return HGS_ERR_INVALID; }
  ShBwdViews v;
  v.n = n_views;
  v.color = 0;
  for (int i = 0; i < HGS_MAX_DEFERRED_VIEWS; ++i) {
    const hgs_sh_bwd_view& w = views[i < n_views ? i : 0];
    if (!w.geom_ws || !w.bwd_ws || !w.campos) { set_error("deferred view %d has a null pointer", i); return HGS_ERR_INVALID; }
    v.mask[i] = GeomWs::carve_from(const_cast<void*>(w.geom_ws), P).tiles_touched;
    v.drgb[i] = BwdWs::carve_from(const_cast<void*>(w.bwd_ws), w.L, P).drgb;
    v.campos[i] = w.campos;
  }
  HGS_HIP(hipSetDevice(device));
  return HGS_TIMED(ST_SH_BATCHED, static_cast<hipStream_t>(stream),
                   launch_sh_bwd_batched(v, P, M, sh_degree, means3D, shs, dL_dshs, dL_dmeans3D, accumulate != 0,
                                         static_cast<hipStream_t>(stream)));
}

static int sh_color_check(const hgs_sh_color_view* views, int32_t n_views, int32_t M, int32_t sh_degree,
                          const float* means3D, const float* shs, bool backward) {
  if (!views || n_views > HGS_MAX_DEFERRED_VIEWS) { set_error("1..%d views per call", HGS_MAX_DEFERRED_VIEWS); return HGS_ERR_INVALID; }
  if (!means3D || !shs) { set_error("null argument"); return HGS_ERR_INVALID; }
  if (sh_degree < 0 || sh_degree > 3 || M < (sh_degree + 1) * (sh_degree + 1) || M > 16) { set_error("M=%d incompatible with sh_degree=%d", M, sh_degree); return HGS_ERR_INVALID; }
  if ((uintptr_t)shs & 15u) { set_error("shs must be 16-byte aligned"); return HGS_ERR_INVALID; }
  for (int i = 0; i < n_views; ++i)
    if (!views[i].campos || !views[i].clamp || (backward ? !views[i].d_rgb : !views[i].rgb)) { set_error("colour view %d has a null pointer", i); return HGS_ERR_INVALID; }
  return HGS_OK;
}

int hgs_sh_colors_batched(const hgs_sh_color_view* views, int32_t n_views, int32_t P, int32_t M, int32_t sh_degree,
                          const float* means3D, const float* shs, hgs_stream_t stream, int device) {
  if (n_views <= 0 || P <= 0) return HGS_OK;
  int rc = sh_color_check(views, n_views, M, sh_degree, means3D, shs, false);
  if (rc) return rc;
  ShFwdViews v;
  v.n = n_views;
  for (int i = 0; i < HGS_MAX_DEFERRED_VIEWS; ++i) {
    const hgs_sh_color_view& w = views[i < n_views ? i : 0];
    v.campos[i] = w.campos;
    v.rgb_out[i] = w.rgb;
    v.clamp_out[i] = w.clamp;
  }
  HGS_HIP(hipSetDevice(device));
  return launch_sh_colors_batched(v, P, M, sh_degree, means3D, shs, static_cast<hipStream_t>(stream));
}

int hgs_sh_colors_batched_bwd(const hgs_sh_color_view* views, int32_t n_views, int32_t P, int32_t M, int32_t sh_degree,
                              const float* means3D, const float* shs, float* dL_dshs, float* dL_dmeans3D,
                              int32_t accumulate, hgs_stream_t stream, int device) {
  if (n_views <= 0 || P <= 0) return HGS_OK;
  if (!dL_dshs || !dL_dmeans3D || ((uintptr_t)dL_dshs & 15u)) { set_error("dL_dshs (16-byte aligned) / dL_dmeans3D missing"); return HGS_ERR_INVALID; }
  int rc = sh_color_check(views, n_views, M, sh_degree, means3D, shs, true);
  if (rc) return rc;
  ShBwdViews v;
  v.n = n_views;
  v.color = 1;
  for (int i = 0; i < HGS_MAX_DEFERRED_VIEWS; ++i) {
    const hgs_sh_color_view& w = views[i < n_views ? i : 0];
    v.mask[i] = w.clamp;
    v.drgb[i] = w.d_rgb;
    v.campos[i] = w.campos;
  }
  HGS_HIP(hipSetDevice(device));
  return HGS_TIMED(ST_SH_BATCHED, static_cast<hipStream_t>(stream),
                   launch_sh_bwd_batched(v, P, M, sh_degree, means3D, shs, dL_dshs, dL_dmeans3D, accumulate != 0,
                                         static_cast<hipStream_t>(stream)));
}

int hgs_raster_views_get(int32_t P, int32_t width, int32_t height, uint32_t L, const void* geom_ws,
                         const void* bin_ws, const void* img_ws, hgs_raster_views* out) {
  if (!out || !geom_ws || !bin_ws || !img_ws) { set_error("null argument"); return HGS_ERR_INVALID; }
  const int T = grid_x(width) * grid_y(height);
  const GeomWs g = GeomWs::carve_from(const_cast<void*>(geom_ws), P);
  const BinWs b = BinWs::carve_from(const_cast<void*>(bin_ws), L, T);
  const ImgWs im = ImgWs::carve_from(const_cast<void*>(img_ws), width, height);
  out->tile_ids_sorted = b.keys_out;
  out->point_list = b.vals_out;
  out->ranges = b.ranges;
  out->tiles_touched = g.tiles_touched;
  out->offsets = g.offsets;
  out->depths = g.depths;
  out->rects = g.rects;
  out->records = g.records;
  out->final_T = im.final_T;
  out->n_contrib = im.n_contrib;
  return HGS_OK;
}

int hgs_timing_enable(int on) {
  std::lock_guard<std::mutex> lk(g_tmu);
  g_timing = (uint32_t)on;
  return HGS_OK;
}
int hgs_timing_stage_count(void) { return ST_COUNT; }
const char* hgs_timing_stage_name(int i) { return (i >= 0 && i < ST_COUNT) ? kStageNames[i] : ""; }
int hgs_timing_read(double* ms_out, uint32_t* calls_out, int reset) {
  std::lock_guard<std::mutex> lk(g_tmu);
  for (const Pending& p : g_pending) {
    float ms = 0.f;
    if (hipEventSynchronize(p.b) == hipSuccess && hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
      g_ms[p.stage] += ms;
      g_calls[p.stage] += 1;
    }
    g_pool.push_back(p.a);
    g_pool.push_back(p.b);
  }
  g_pending.clear();
  for (int i = 0; i < ST_COUNT; ++i) {
    if (ms_out) ms_out[i] = g_ms[i];
    if (calls_out) calls_out[i] = g_calls[i];
    if (reset) { g_ms[i] = 0.0; g_calls[i] = 0; }
  }
  return HGS_OK;
}

size_t hgs_sort_tmp_bytes(uint32_t n) { return sort_tmp_bytes(n ? n : 1); }

int hgs_sort_pairs(const uint64_t* keys_in, const uint32_t* vals_in, uint64_t* keys_out, uint32_t* vals_out,
                   void* tmp, uint32_t n, int end_bit, hgs_stream_t stream, int device) {
  if (n && (!keys_in || !vals_in || !keys_out || !vals_out || !tmp)) { set_error("null argument"); return HGS_ERR_INVALID; }
  HGS_HIP(hipSetDevice(device));
  return sort_pairs(keys_in, vals_in, keys_out, vals_out, tmp, n, end_bit, static_cast<hipStream_t>(stream), false);
}

constexpr int32_t kHierBuildMaxP = 1 << 30;
constexpr int64_t kHierMaxNodes = 0x7fffffff;   // merge, align, trim and transform: node indices are int32
constexpr int64_t kHierReachMaxRegions = 1 << 24;   // view regions of one hgs_hier_reach call

// The workspace pointer of a hierarchy call: there, and kAlign-aligned (those workspaces are carved without slack).
static int check_hier_tmp(const void* tmp) {
  if (!tmp) { set_error("null argument"); return HGS_ERR_INVALID; }
  if ((uintptr_t)tmp & (kAlign - 1)) { set_error("tmp must be %d-byte aligned", (int)kAlign); return HGS_ERR_INVALID; }
  return HGS_OK;
}

// shs may move in 16-byte pieces: 12 M a multiple of 16 and both bases aligned
static bool shs16_ok(const hgs_hier_view* in, const hgs_hier_view* out) {
  return (3 * in->M) % 4 == 0 && (((uintptr_t)in->shs | (uintptr_t)out->shs) & 15u) == 0;
}

size_t hgs_hier_build_tmp_bytes(int32_t P) {
  if (P < 1 || P > kHierBuildMaxP) return 0;
  return hier_build_tmp_bytes(P);
}

int hgs_hier_build(const float* xyz, const float* scales, const float* rots, const float* opacity, const float* shs,
                   int32_t P, int32_t M, float* out_xyz, float* out_shs, float* out_alpha, float* out_log_scales,
                   float* out_rots, int32_t* out_nodes, float* out_boxes, void* tmp, hgs_stream_t stream, int device) {
  if (P < 1 || P > kHierBuildMaxP) { set_error("bad sizes: P=%d not in [1, 2^30]", P); return HGS_ERR_INVALID; }
  if (M != 1 && M != 4 && M != 9 && M != 16) { set_error("bad sizes: M=%d not in {1, 4, 9, 16}", M); return HGS_ERR_INVALID; }
  if (!xyz || !scales || !rots || !opacity || !shs || !out_xyz || !out_shs || !out_alpha || !out_log_scales ||
      !out_rots || !out_nodes || !out_boxes || !tmp) {
    set_error("null argument");
    return HGS_ERR_INVALID;
  }
  if (((uintptr_t)out_shs | (uintptr_t)out_rots | (uintptr_t)out_boxes) & 15u) { set_error("out_shs / out_rots / out_boxes must be 16-byte aligned"); return HGS_ERR_INVALID; }
  if (int rc = check_hier_tmp(tmp)) return rc;
  HGS_HIP(hipSetDevice(device));
  return launch_hier_build(xyz, scales, rots, opacity, shs, P, M, out_xyz, out_shs, out_alpha, out_log_scales, out_rots,
                           out_nodes, out_boxes, tmp, static_cast<hipStream_t>(stream));
}

static int check_merged_view(const hgs_hier_view* merged, int32_t k) {
  if (k < 1) { set_error("bad sizes: k=%d chunks < 1", k); return HGS_ERR_INVALID; }
  if (merged->N < 1 + (int64_t)k || merged->N > kHierMaxNodes) {
    set_error("bad sizes: merged N=%lld not in [1 + k, 2^31 - 1] (k=%d)", (long long)merged->N, k);
    return HGS_ERR_INVALID;
  }
  if (merged->G != merged->N) { set_error("bad sizes: merged G=%lld != N=%lld", (long long)merged->G, (long long)merged->N); return HGS_ERR_INVALID; }
  if (merged->M < 1 || merged->M > 64) { set_error("bad sizes: merged M=%d not in [1, 64]", merged->M); return HGS_ERR_INVALID; }
  return HGS_OK;
}

static bool null_view(const hgs_hier_view* v) {
  return !v->xyz || !v->shs || !v->alpha || !v->log_scales || !v->rots || !v->nodes || !v->boxes;
}

int hgs_hier_merge_place(const hgs_hier_view* chunk, int32_t index, int32_t k, int64_t base, const hgs_hier_view* merged,
                         void* tmp, hgs_hier_merge_report* report, hgs_stream_t stream, int device) {
  if (!chunk || !merged || !report) { set_error("null argument"); return HGS_ERR_INVALID; }
  if (chunk->N < 1 || chunk->N > kHierMaxNodes) { set_error("bad sizes: chunk N=%lld not in [1, 2^31 - 1]", (long long)chunk->N); return HGS_ERR_INVALID; }
  if (chunk->G < chunk->N) { set_error("bad sizes: chunk G=%lld < N=%lld", (long long)chunk->G, (long long)chunk->N); return HGS_ERR_INVALID; }
  int rc = check_merged_view(merged, k);
  if (rc) return rc;
  if (chunk->M != merged->M) { set_error("bad sizes: chunk M=%d != merged M=%d", chunk->M, merged->M); return HGS_ERR_INVALID; }
  if (index < 0 || index >= k) { set_error("bad sizes: chunk index=%d not in [0, k=%d)", index, k); return HGS_ERR_INVALID; }
  if (base < 1 + (int64_t)k || base > merged->N - chunk->N + 1) {
    set_error("bad sizes: base=%lld not in [1 + k, merged N - chunk N + 1] = [%lld, %lld]", (long long)base,
              (long long)(1 + (int64_t)k), (long long)(merged->N - chunk->N + 1));
    return HGS_ERR_INVALID;
  }
  if (null_view(chunk) || null_view(merged) || !tmp) { set_error("null argument"); return HGS_ERR_INVALID; }
  HGS_HIP(hipSetDevice(device));
  return launch_hier_merge_place(*chunk, index, base, *merged, tmp, report, static_cast<hipStream_t>(stream));
}

int hgs_hier_merge_root(const hgs_hier_view* merged, int32_t k, hgs_stream_t stream, int device) {
  if (!merged) { set_error("null argument"); return HGS_ERR_INVALID; }
  int rc = check_merged_view(merged, k);
  if (rc) return rc;
  if (null_view(merged)) { set_error("null argument"); return HGS_ERR_INVALID; }
  if (((uintptr_t)merged->rots | (uintptr_t)merged->boxes) & 15u) { set_error("merged rots / boxes must be 16-byte aligned"); return HGS_ERR_INVALID; }
  HGS_HIP(hipSetDevice(device));
  return launch_hier_merge_root(*merged, k, static_cast<hipStream_t>(stream));
}

size_t hgs_hier_align_tmp_bytes(int64_t N) {
  if (N < 1 || N > kHierMaxNodes) return 0;
  return hier_align_tmp_bytes(N);
}

int hgs_hier_align(const int32_t* nodes, int64_t N, float* log_scales, float* rots, void* tmp,
                   hgs_hier_align_report* report, hgs_stream_t stream, int device) {
  if (N < 1 || N > kHierMaxNodes) { set_error("bad sizes: N=%lld not in [1, 2^31 - 1]", (long long)N); return HGS_ERR_INVALID; }
  if (!nodes || !log_scales || !rots || !tmp || !report) { set_error("null argument"); return HGS_ERR_INVALID; }
  if ((uintptr_t)rots & 15u) { set_error("rots must be 16-byte aligned"); return HGS_ERR_INVALID; }
  if (int rc = check_hier_tmp(tmp)) return rc;
  HGS_HIP(hipSetDevice(device));
  return launch_hier_align(nodes, N, log_scales, rots, tmp, report, static_cast<hipStream_t>(stream));
}

size_t hgs_hier_trim_tmp_bytes(int64_t N) {
  if (N < 1 || N > kHierMaxNodes) return 0;
  return hier_trim_tmp_bytes(N);
}

// Sizes, pointers and alignment of one side of a trim or transform call.
static int check_hier_view(const hgs_hier_view* v, const char* side) {
  if (v->N < 1 || v->N > kHierMaxNodes) { set_error("bad sizes: %s N=%lld not in [1, 2^31 - 1]", side, (long long)v->N); return HGS_ERR_INVALID; }
  if (v->G < v->N) { set_error("bad sizes: %s G=%lld < N=%lld", side, (long long)v->G, (long long)v->N); return HGS_ERR_INVALID; }
  if (v->M < 1 || v->M > 64) { set_error("bad sizes: %s M=%d not in [1, 64]", side, v->M); return HGS_ERR_INVALID; }
  if (null_view(v)) { set_error("null argument"); return HGS_ERR_INVALID; }
  if (((uintptr_t)v->rots | (uintptr_t)v->boxes) & 15u) { set_error("%s rots / boxes must be 16-byte aligned", side); return HGS_ERR_INVALID; }
  if (((uintptr_t)v->xyz | (uintptr_t)v->shs | (uintptr_t)v->alpha | (uintptr_t)v->log_scales | (uintptr_t)v->nodes) & 3u) {
    set_error("%s xyz / shs / alpha / log_scales / nodes must be 4-byte aligned", side);
    return HGS_ERR_INVALID;
  }
  return HGS_OK;
}

// The two trim plan calls.  keyed: key has to be there and aligned, and key_floor a number.
static int hier_trim_plan(const hgs_hier_view* in, const hgs_hier_trim_args* args, bool keyed, const float* key,
                          float key_floor, void* tmp, hgs_hier_trim_report* report, hgs_stream_t stream, int device) {
  if (!in || !args || !report || (keyed && !key)) { set_error("null argument"); return HGS_ERR_INVALID; }
  int rc = check_hier_view(in, "input");
  if (rc) return rc;
  if (keyed && ((uintptr_t)key & 3u)) { set_error("key must be 4-byte aligned"); return HGS_ERR_INVALID; }
  bool nan = std::isnan(args->min_extent) || (keyed && std::isnan(key_floor));
  for (int a = 0; a < 3 && args->use_roi; ++a) nan = nan || std::isnan(args->roi_lo[a]) || std::isnan(args->roi_hi[a]);
  if (nan) {
    set_error(keyed ? "min_extent, key_floor or a region bound is NaN" : "min_extent or a region bound is NaN");
    return HGS_ERR_INVALID;
  }
  if ((rc = check_hier_tmp(tmp))) return rc;
  for (int k = 0; k < 4; ++k) report->first_bad[k] = -1;
  report->kept = report->stubs = 0;
  HGS_HIP(hipSetDevice(device));
  return launch_hier_trim_plan(*in, *args, key, key_floor, tmp, report, static_cast<hipStream_t>(stream), device);
}

int hgs_hier_trim_plan(const hgs_hier_view* in, const hgs_hier_trim_args* args, void* tmp, hgs_hier_trim_report* report,
                       hgs_stream_t stream, int device) {
  return hier_trim_plan(in, args, false, nullptr, 0.0f, tmp, report, stream, device);
}

int hgs_hier_trim_plan_keyed(const hgs_hier_view* in, const hgs_hier_trim_args* args, const float* key, float key_floor,
                             void* tmp, hgs_hier_trim_report* report, hgs_stream_t stream, int device) {
  return hier_trim_plan(in, args, true, key, key_floor, tmp, report, stream, device);
}

// What hgs_hier_trim_apply and hgs_hier_prune_apply check in common, in the order they always had: first the views, M,
// tmp and the maps ...
static int check_hier_apply_args(const hgs_hier_view* in, const hgs_hier_view* out, const void* tmp,
                                 const int32_t* old_of_new, const int32_t* new_of_old) {
  if (!in || !out) { set_error("null argument"); return HGS_ERR_INVALID; }
  int rc = check_hier_view(in, "input");
  if (!rc) rc = check_hier_view(out, "output");
  if (rc) return rc;
  if (in->M != out->M) { set_error("bad sizes: input M=%d != output M=%d", in->M, out->M); return HGS_ERR_INVALID; }
  if (!tmp || !old_of_new || !new_of_old) { set_error("null argument"); return HGS_ERR_INVALID; }
  if ((rc = check_hier_tmp(tmp))) return rc;
  if (((uintptr_t)old_of_new | (uintptr_t)new_of_old) & 3u) { set_error("old_of_new / new_of_old must be 4-byte aligned"); return HGS_ERR_INVALID; }
  return HGS_OK;
}

// ... then (behind prune's mode check) the sizes against the plan's.  planned: the tool's lookup; plan_call: its name.
static int check_hier_apply_plan(const hgs_hier_view* in, const hgs_hier_view* out, const void* tmp, int device,
                                 bool (*planned)(int, const void*, int64_t*, int64_t*), const char* plan_call) {
  int64_t planned_N = 0, kept = 0;
  if (!planned(device, tmp, &planned_N, &kept)) {
    set_error("no successful %s on this device and tmp", plan_call);
    return HGS_ERR_INVALID;
  }
  if (in->N != planned_N) { set_error("bad sizes: input N=%lld, the plan was made for N=%lld", (long long)in->N, (long long)planned_N); return HGS_ERR_INVALID; }
  if (out->N != kept) { set_error("bad sizes: output N=%lld != the plan's kept count %lld", (long long)out->N, (long long)kept); return HGS_ERR_INVALID; }
  return HGS_OK;
}

// The first of the seven arrays of `out` that overlaps its array of `in` -> its name; nullptr: none does.  g_*: the rows
// of the five arrays of Gaussians, n_*: the rows of nodes and boxes.  same_ok: an output array may BE its input array.
static const char* overlapping_hier_array(const hgs_hier_view* in, size_t g_in, size_t n_in, const hgs_hier_view* out,
                                          size_t g_out, size_t n_out, bool same_ok) {
  const struct { const void* a; const void* b; size_t row; bool node; const char* name; } pairs[7] = {
      {in->xyz, out->xyz, 12, false, "xyz"}, {in->shs, out->shs, 12 * (size_t)in->M, false, "shs"},
      {in->alpha, out->alpha, 4, false, "alpha"}, {in->log_scales, out->log_scales, 12, false, "log_scales"},
      {in->rots, out->rots, 16, false, "rots"}, {in->nodes, out->nodes, 28, true, "nodes"},
      {in->boxes, out->boxes, 32, true, "boxes"}};
  for (const auto& pr : pairs) {
    const uintptr_t a = (uintptr_t)pr.a, b = (uintptr_t)pr.b;
    if (same_ok && a == b) continue;
    if (a < b + (pr.node ? n_out : g_out) * pr.row && b < a + (pr.node ? n_in : g_in) * pr.row) return pr.name;
  }
  return nullptr;
}

size_t hgs_hier_reach_tmp_bytes(int64_t N, int64_t C) {
  if (N < 1 || N > kHierMaxNodes || C < 1 || C > kHierReachMaxRegions) return 0;
  return hier_reach_tmp_bytes(N, (int32_t)C);
}

int hgs_hier_reach(const float* boxes, int64_t N, const float* regions, int64_t C, float* reach, void* tmp,
                   hgs_stream_t stream, int device) {
  if (N < 1 || N > kHierMaxNodes) { set_error("bad sizes: N=%lld not in [1, 2^31 - 1]", (long long)N); return HGS_ERR_INVALID; }
  if (C < 1 || C > kHierReachMaxRegions) { set_error("bad sizes: C=%lld regions not in [1, 2^24]", (long long)C); return HGS_ERR_INVALID; }
  if (!boxes || !regions || !reach) { set_error("null argument"); return HGS_ERR_INVALID; }
  if ((uintptr_t)boxes & 15u) { set_error("boxes must be 16-byte aligned"); return HGS_ERR_INVALID; }
  if (((uintptr_t)regions | (uintptr_t)reach) & 3u) { set_error("regions / reach must be 4-byte aligned"); return HGS_ERR_INVALID; }
  if (int rc = check_hier_tmp(tmp)) return rc;
  HGS_HIP(hipSetDevice(device));
  return launch_hier_reach(boxes, N, regions, (int32_t)C, reach, tmp, static_cast<hipStream_t>(stream));
}

int hgs_hier_trim_apply(const hgs_hier_view* in, const hgs_hier_view* out, const void* tmp, int32_t* old_of_new,
                        int32_t* new_of_old, hgs_stream_t stream, int device) {
  int rc = check_hier_apply_args(in, out, tmp, old_of_new, new_of_old);
  if (!rc) rc = check_hier_apply_plan(in, out, tmp, device, hier_trim_planned, "hgs_hier_trim_plan");
  if (rc) return rc;
  HGS_HIP(hipSetDevice(device));
  return launch_hier_trim_apply(*in, *out, tmp, old_of_new, new_of_old, shs16_ok(in, out), static_cast<hipStream_t>(stream));
}

// The renderer's SH basis of bands 1..3 at a unit direction (hgs.hierarchy.sh_band_basis), b[0..3), b[3..8), b[8..15).
static void sh_band_basis(const double d[3], double b[15]) {
  const double x = d[0], y = d[1], z = d[2];
  const double xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
  const double C1 = 0.4886025119029199;
  b[0] = -C1 * y; b[1] = C1 * z; b[2] = -C1 * x;
  b[3] = 1.0925484305920792 * xy; b[4] = -1.0925484305920792 * yz; b[5] = 0.31539156525252005 * (2.0 * zz - xx - yy);
  b[6] = -1.0925484305920792 * xz; b[7] = 0.5462742152960396 * (xx - yy);
  b[8] = -0.5900435899266435 * y * (3 * xx - yy); b[9] = 2.890611442640554 * xy * z;
  b[10] = -0.4570457994644658 * y * (4 * zz - xx - yy); b[11] = 0.3731763325901154 * z * (2 * zz - 3 * xx - 3 * yy);
  b[12] = -0.4570457994644658 * x * (4 * zz - xx - yy); b[13] = 1.445305721320277 * z * (xx - yy);
  b[14] = -0.5900435899266435 * x * (xx - 3 * yy);
}

// The parameter block of a similarity transform: everything hgs.h lists, on the host.
static int check_transform_args(const hgs_hier_transform_args* a) {
  bool finite = std::isfinite(a->s) && std::isfinite(a->log_s);
  for (int k = 0; k < 3; ++k) finite = finite && std::isfinite(a->t[k]);
  if (!finite || !(a->s > 0.0)) { set_error("bad transform: s and t must be finite and s > 0"); return HGS_ERR_INVALID; }
  if (!(std::fabs(a->log_s - std::log(a->s)) <= 1e-12)) { set_error("bad transform: log_s is not log(s)"); return HGS_ERR_INVALID; }
  const double* R = a->R;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      const double dot = R[3 * i] * R[3 * j] + R[3 * i + 1] * R[3 * j + 1] + R[3 * i + 2] * R[3 * j + 2];
      if (!(std::fabs(dot - (i == j ? 1.0 : 0.0)) <= 1e-9)) { set_error("bad transform: R is not orthonormal (|R R^T - I| > 1e-9)"); return HGS_ERR_INVALID; }
    }
  const double det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
  if (!(det > 0.0)) { set_error("bad transform: det R < 0 (a mirror)"); return HGS_ERR_INVALID; }
  const double w = a->q[0], x = a->q[1], y = a->q[2], z = a->q[3];
  const double Rq[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                        2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)};
  for (int k = 0; k < 9; ++k)
    if (!(std::fabs(Rq[k] - R[k]) <= 1e-9)) { set_error("bad transform: q does not reproduce R"); return HGS_ERR_INVALID; }
  const double* D[3] = {a->D1, a->D2, a->D3};
  for (int l = 1; l <= 3; ++l) {
    const int n = 2 * l + 1;
    const double* Dl = D[l - 1];
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < n; ++j) {
        double dot = 0.0;
        for (int k = 0; k < n; ++k) dot += Dl[i * n + k] * Dl[j * n + k];
        if (!(std::fabs(dot - (i == j ? 1.0 : 0.0)) <= 1e-9)) { set_error("bad transform: D%d is not orthogonal", l); return HGS_ERR_INVALID; }
      }
  }
  // consistency with R at 16 fixed directions (a Fibonacci sphere): D_l^T b_l(d) = b_l(R^T d)
  for (int i = 0; i < 16; ++i) {
    const double zc = 1.0 - (2.0 * i + 1.0) / 16.0, r = std::sqrt(1.0 - zc * zc), phi = i * 2.399963229728653;
    const double d[3] = {r * std::cos(phi), r * std::sin(phi), zc};
    const double dr[3] = {R[0] * d[0] + R[3] * d[1] + R[6] * d[2], R[1] * d[0] + R[4] * d[1] + R[7] * d[2],
                          R[2] * d[0] + R[5] * d[1] + R[8] * d[2]};
    double b[15], br[15];
    sh_band_basis(d, b);
    sh_band_basis(dr, br);
    for (int l = 1; l <= 3; ++l) {
      const int n = 2 * l + 1, o = l * l - 1;
      const double* Dl = D[l - 1];
      for (int j = 0; j < n; ++j) {
        double v = 0.0;
        for (int k = 0; k < n; ++k) v += Dl[k * n + j] * b[o + k];
        if (!(std::fabs(v - br[o + j]) <= 1e-9)) { set_error("bad transform: D%d is not the SH block of R", l); return HGS_ERR_INVALID; }
      }
    }
  }
  return HGS_OK;
}

int hgs_hier_transform(const hgs_hier_view* in, const hgs_hier_view* out, const hgs_hier_transform_args* args,
                       hgs_stream_t stream, int device) {
  if (!in || !out || !args) { set_error("null argument"); return HGS_ERR_INVALID; }
  int rc = check_hier_view(in, "input");
  if (!rc) rc = check_hier_view(out, "output");
  if (rc) return rc;
  if (in->G > kHierMaxNodes) { set_error("bad sizes: G=%lld > 2^31 - 1", (long long)in->G); return HGS_ERR_INVALID; }
  if (in->G != out->G || in->N != out->N || in->M != out->M) {
    set_error("bad sizes: input (G=%lld, N=%lld, M=%d) != output (G=%lld, N=%lld, M=%d)", (long long)in->G, (long long)in->N,
              in->M, (long long)out->G, (long long)out->N, out->M);
    return HGS_ERR_INVALID;
  }
  if (in->M != 1 && in->M != 4 && in->M != 9 && in->M != 16) { set_error("bad sizes: M=%d not in {1, 4, 9, 16} (whole SH bands only)", in->M); return HGS_ERR_INVALID; }
  // every output array is its input array (in place) or does not overlap it
  const size_t G = (size_t)in->G, N = (size_t)in->N;
  if (const char* name = overlapping_hier_array(in, G, N, out, G, N, true)) {
    set_error("output %s overlaps input %s without being the same array", name, name);
    return HGS_ERR_INVALID;
  }
  rc = check_transform_args(args);
  if (rc) return rc;
  HGS_HIP(hipSetDevice(device));
  return launch_hier_transform(*in, *out, *args, shs16_ok(in, out), static_cast<hipStream_t>(stream));
}

size_t hgs_hier_refit_tmp_bytes(int64_t N) {
  if (N < 1 || N > kHierMaxNodes) return 0;
  return hier_refit_tmp_bytes(N);
}

int hgs_hier_refit(const hgs_hier_view* in, float* boxes_out, int32_t leaf_mode, void* tmp, hgs_hier_refit_report* report,
                   hgs_stream_t stream, int device) {
  if (!in || !boxes_out || !report) { set_error("null argument"); return HGS_ERR_INVALID; }
  int rc = check_hier_view(in, "input");
  if (rc) return rc;
  if ((uintptr_t)boxes_out & 15u) { set_error("boxes_out must be 16-byte aligned"); return HGS_ERR_INVALID; }
  // boxes_out is the input's boxes (in place) or does not overlap them
  const uintptr_t a = (uintptr_t)in->boxes, b = (uintptr_t)boxes_out;
  const size_t bytes = (size_t)in->N * 32;
  if (a != b && a < b + bytes && b < a + bytes) {
    set_error("boxes_out overlaps the input boxes without being the same array");
    return HGS_ERR_INVALID;
  }
  if (leaf_mode < 0 || leaf_mode > 2) { set_error("bad leaf mode %d: 0 (keep), 1 (cube) or 2 (ellipsoid) expected", leaf_mode); return HGS_ERR_INVALID; }
  if ((rc = check_hier_tmp(tmp))) return rc;
  for (int k = 0; k < 7; ++k) report->first_bad[k] = -1;
  report->levels = 0;
  report->leaves = report->children_sum = 0;
  HGS_HIP(hipSetDevice(device));
  return launch_hier_refit(*in, boxes_out, leaf_mode, tmp, report, static_cast<hipStream_t>(stream));
}

size_t hgs_hier_prune_tmp_bytes(int64_t N) {
  if (N < 1 || N > kHierMaxNodes) return 0;
  return hier_prune_tmp_bytes(N);
}

int hgs_hier_prune_plan(const hgs_hier_view* in, const hgs_hier_prune_args* args, const uint8_t* remove, void* tmp,
                        hgs_hier_prune_report* report, hgs_stream_t stream, int device) {
  if (!in || !args || !report) { set_error("null argument"); return HGS_ERR_INVALID; }
  int rc = check_hier_view(in, "input");
  if (rc) return rc;
  if (args->remove_boxes < 0 || args->remove_boxes > HGS_HIER_PRUNE_MAX_BOXES) {
    set_error("bad criteria: %d remove boxes, 0 .. %d expected", args->remove_boxes, HGS_HIER_PRUNE_MAX_BOXES);
    return HGS_ERR_INVALID;
  }
  bool nan = (args->use_min_opacity && std::isnan(args->min_opacity)) || (args->use_max_scale && std::isnan(args->log_max_scale));
  for (int b = 0; b < args->remove_boxes; ++b)
    for (int a = 0; a < 3; ++a) nan = nan || std::isnan(args->remove_lo[b][a]) || std::isnan(args->remove_hi[b][a]);
  for (int a = 0; a < 3 && args->use_keep_box; ++a) nan = nan || std::isnan(args->keep_lo[a]) || std::isnan(args->keep_hi[a]);
  if (nan) { set_error("bad criteria: a box bound, min_opacity or log_max_scale is NaN"); return HGS_ERR_INVALID; }
  if ((rc = check_hier_tmp(tmp))) return rc;
  for (int k = 0; k < 6; ++k) report->first_bad[k] = -1;
  report->levels = report->root_dead = 0;
  report->kept = report->removed_leaves = report->dead = report->dirty = report->single_child = report->children_sum = 0;
  HGS_HIP(hipSetDevice(device));
  return launch_hier_prune_plan(*in, *args, remove, tmp, report, static_cast<hipStream_t>(stream), device);
}

int hgs_hier_prune_apply(const hgs_hier_view* in, const hgs_hier_view* out, const void* tmp, int32_t remerge,
                         int32_t* old_of_new, int32_t* new_of_old, hgs_stream_t stream, int device) {
  int rc = check_hier_apply_args(in, out, tmp, old_of_new, new_of_old);
  if (rc) return rc;
  if (remerge < HGS_HIER_PRUNE_REMERGE_NONE || remerge > HGS_HIER_PRUNE_REMERGE_ALL) {
    set_error("bad remerge mode %d: 0 (none), 1 (dirty) or 2 (all) expected", remerge);
    return HGS_ERR_INVALID;
  }
  if ((rc = check_hier_apply_plan(in, out, tmp, device, hier_prune_planned, "hgs_hier_prune_plan"))) return rc;
  // no output array overlaps its input array (the rows the input shows: N of them)
  const size_t nin = (size_t)in->N, nout = (size_t)out->N;
  if (const char* name = overlapping_hier_array(in, nin, nin, out, nout, nout, false)) {
    set_error("output %s overlaps input %s", name, name);
    return HGS_ERR_INVALID;
  }
  HGS_HIP(hipSetDevice(device));
  return launch_hier_prune_apply(*in, *out, tmp, remerge, old_of_new, new_of_old, shs16_ok(in, out),
                                 static_cast<hipStream_t>(stream), device);
}

size_t hgs_ssim_tmp_bytes(int32_t N, int32_t C, int32_t H, int32_t W) {
  if (!ssim_sizes_ok(N, C, H, W)) return 0;
  return ssim_tmp_bytes(N, C, H, W);
}

int hgs_ssim_fwd(const float* img1, const float* img2, int32_t N, int32_t C, int32_t H, int32_t W, float* out_image,
                 float* out_mean, float* maps, void* tmp, hgs_stream_t stream, int device) {
  if (!ssim_sizes_ok(N, C, H, W)) return HGS_ERR_INVALID;
  if (!img1 || !img2 || !out_image || !out_mean || !tmp) { set_error("null argument"); return HGS_ERR_INVALID; }
  if ((uintptr_t)tmp & 7u) { set_error("tmp must be 8-byte aligned"); return HGS_ERR_INVALID; }
  HGS_HIP(hipSetDevice(device));
  return launch_ssim_fwd(img1, img2, N, C, H, W, out_image, out_mean, maps, tmp, static_cast<hipStream_t>(stream));
}

int hgs_ssim_bwd(const float* img1, const float* img2, const float* maps, const float* grad_out, int32_t per_image,
                 int32_t N, int32_t C, int32_t H, int32_t W, float* grad_img1, hgs_stream_t stream, int device) {
  if (!ssim_sizes_ok(N, C, H, W)) return HGS_ERR_INVALID;
  if (!img1 || !img2 || !maps || !grad_out || !grad_img1) { set_error("null argument"); return HGS_ERR_INVALID; }
  HGS_HIP(hipSetDevice(device));
  return launch_ssim_bwd(img1, img2, maps, grad_out, per_image, N, C, H, W, grad_img1,
                         static_cast<hipStream_t>(stream));
}

// Everything hgs_photo_fwd / hgs_photo_bwd can refuse without touching the device.
static bool photo_args_ok(const hgs_photo_args* a, const void* tmp) {
  if (!a) { set_error("null argument"); return false; }
  if (!ssim_sizes_ok(a->N, a->C, a->H, a->W)) return false;
  if (a->exposure && a->C != 3) { set_error("bad sizes: C=%d with an exposure (a 3x4 exposure needs C = 3)", a->C); return false; }
  if (!a->rendered || !a->gt || !tmp) { set_error("null argument"); return false; }
  if (((a->invdepth != nullptr) != (a->mono_invdepth != nullptr)) || ((a->invdepth != nullptr) != (a->depth_mask != nullptr))) {
    set_error("incomplete depth triple: invdepth, mono_invdepth and depth_mask are given all three or none");
    return false;
  }
  if (!(a->lambda_dssim >= 0.0 && a->lambda_dssim <= 1.0)) { set_error("lambda_dssim=%g not in [0, 1]", a->lambda_dssim); return false; }
  if (!std::isfinite(a->depth_weight)) { set_error("depth_weight=%g is not finite", a->depth_weight); return false; }
  if ((uintptr_t)tmp & 7u) { set_error("tmp must be 8-byte aligned"); return false; }
  return true;
}

size_t hgs_photo_tmp_bytes(int32_t N, int32_t C, int32_t H, int32_t W) {
  if (!ssim_sizes_ok(N, C, H, W)) return 0;
  return photo_tmp_bytes(N, C, H, W);
}

int hgs_photo_fwd(const hgs_photo_args* args, float* out, float* maps, void* tmp, hgs_stream_t stream, int device) {
  if (!photo_args_ok(args, tmp)) return HGS_ERR_INVALID;
  if (!out) { set_error("null argument"); return HGS_ERR_INVALID; }
  HGS_HIP(hipSetDevice(device));
  return launch_photo_fwd(*args, out, maps, tmp, static_cast<hipStream_t>(stream));
}

int hgs_photo_bwd(const hgs_photo_args* args, const float* maps, const float* grad_out, float* grad_rendered,
                  float* grad_exposure, float* grad_invdepth, void* tmp, hgs_stream_t stream, int device) {
  if (!photo_args_ok(args, tmp)) return HGS_ERR_INVALID;
  if (!maps || !grad_out || !grad_rendered) { set_error("null argument"); return HGS_ERR_INVALID; }
  if (grad_exposure && !args->exposure) { set_error("grad_exposure without an exposure"); return HGS_ERR_INVALID; }
  if (grad_invdepth && !args->invdepth) { set_error("grad_invdepth without an invdepth"); return HGS_ERR_INVALID; }
  HGS_HIP(hipSetDevice(device));
  return launch_photo_bwd(*args, maps, grad_out, grad_rendered, grad_exposure, grad_invdepth, tmp,
                          static_cast<hipStream_t>(stream));
}

}  // extern "C"
