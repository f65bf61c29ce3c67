/*
 * hgs.h -- C ABI of libhgs.so, the MI355X (gfx950) implementation of the
 * hierarchical-3D-Gaussian rasterizer hot path.
 *
 * Plain C: raw device pointers, sizes and a hipStream_t passed as void*.  No
 * torch / C++ types cross this boundary.  Every entry point below names the
 * reference interface it stands in for (paths relative to the reference
 * checkout, graphdeco-inria/hierarchical-3d-gaussians):
 *
 *   diff_gaussian_rasterization._C   (submodules/hierarchy-rasterizer, .gitmodules:4-6;
 *                                     imported at gaussian_renderer/__init__.py:14,17)
 *   gaussian_hierarchy._C            (submodules/gaussianhierarchy, .gitmodules:10-12;
 *                                     imported at train_post.py:26, render_hierarchy.py:27,
 *                                     scene/gaussian_model.py:24)
 *   simple_knn._C                    (submodules/simple-knn, .gitmodules:7-9;
 *                                     imported at scene/gaussian_model.py:21)
 *
 * Conventions
 *   - return value 0 = success; anything else is an error code and
 *     hgs_last_error() (thread-local) holds the message;
 *   - every function that touches the GPU takes (stream, device) and calls
 *     hipSetDevice(device) first -- backward runs on an autograd worker thread;
 *   - all device buffers are caller-owned (torch's caching allocator in the
 *     Python host); the library keeps no pointer after a call returns;
 *   - matrices are the reference's stored (row-vector convention) [4,4]
 *     float32 tensors, i.e. column-major standard matrices
 *     (scene/cameras.py:95-97).
 */
#ifndef HGS_H
#define HGS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HGS_ABI_VERSION 14
#define HGS_TILE 16
#define HGS_INST_GRAD_STRIDE 10 /* floats per (tile, Gaussian) instance in the backward scratch (40 bytes: the ten sums) */

enum {
  HGS_OK = 0,
  HGS_ERR_INVALID = 1, /* bad argument */
  HGS_ERR_HIP = 2,     /* a HIP runtime call or kernel failed */
  HGS_ERR_IO = 3,      /* file I/O */
  HGS_ERR_NOMEM = 4,
  HGS_ERR_CAPACITY = 5 /* hgs_raster_fwd: L exceeded the caller's capacity; redo with stage1/stage2 */
};

typedef void* hgs_stream_t; /* hipStream_t */

int hgs_abi_version(void);
const char* hgs_last_error(void);
/* number of HIP devices visible; <0 on error.  Used by the host to fail loudly. */
int hgs_device_count(void);

/* ---------------------------------------------------------------------------
 * Rasterizer.  Replaces diff_gaussian_rasterization._C.rasterize_gaussians /
 * rasterize_gaussians_backward as called through GaussianRasterizer.forward
 * (gaussian_renderer/__init__.py:64,105-113; :267-277; :339,381-389) with the
 * settings of GaussianRasterizationSettings (:44-62).
 * ------------------------------------------------------------------------- */
typedef struct hgs_raster_args {
  int32_t P;          /* Gaussians passed to the op */
  int32_t M;          /* SH coefficients stored per Gaussian ((max_sh_degree+1)^2), 0 with colors_precomp */
  int32_t sh_degree;  /* active degree 0..3 */
  int32_t width, height;
  float tanfovx, tanfovy;
  float scale_modifier;
  int32_t do_depth;   /* write the inverse-depth channel */
  int32_t debug;      /* synchronise + check after every launch */
  int32_t accumulate_grads; /* backward: add into the gradient buffers instead of overwriting them (accumulation over
                             * the views of one optimizer step); dL_dmeans2D and dL_dcolors are per-view quantities
                             * and are always overwritten */
  const float* bg;          /* device [3] */
  const float* viewmatrix;  /* device [16] */
  const float* projmatrix;  /* device [16] */
  const float* campos;      /* device [3] */
  const float* means3D;         /* [P,3] */
  const float* shs;             /* [P,M,3] or NULL */
  const float* colors_precomp;  /* [P,3]  or NULL (exactly one of shs / colors_precomp) */
  const float* opacities;       /* [P] */
  const float* scales;          /* [P,3] or NULL */
  const float* rotations;       /* [P,4] or NULL */
  const float* cov3D_precomp;   /* [P,6] or NULL (exactly one of scales+rotations / cov3D_precomp) */
  const float* interpolation_weights; /* [>=P] or NULL : hierarchy mode (gaussian_renderer/__init__.py:262) */
  const int32_t* num_node_kids;       /* [>=P] or NULL : hierarchy mode (gaussian_renderer/__init__.py:263) */
  /* Raw-parameter fast path: the op applies the activations of
   * scene/gaussian_model.py:108-128 itself, so the caller passes the optimiser's raw tensors and gets gradients
   * w.r.t. them -- no exp / normalize / sigmoid / cat kernels (and their backward) around the op. */
  const float* shs_rest;    /* NULL: shs is [P,M,3].  Else shs = features_dc [P,1,3], shs_rest = features_rest
                             * [P,M-1,3] (the two tensors get_features concatenates, scene/gaussian_model.py:121-124) */
  int32_t activations;      /* OR of HGS_ACT_*; 0 = inputs are already activated (the reference's call) */
  int32_t defer_sh_bwd;     /* backward: skip the SH part (dL_dshs and the view-direction term of dL_dmeans3D); the
                             * caller finishes it for several views at once with hgs_raster_sh_bwd_batched */
  /* ABI 7 (the eight bytes that held a pointer until ABI 4 and nothing since): how non-empty interpolation_weights /
   * num_node_kids are used.  0 (default): a per-GAUSSIAN remap of the opacity in the per-Gaussian kernel,
   *     o' = w o + (1 - w) (1 - (1 - min(o, 0.99))^(1/k))   for k >= 2;
   * 1: the same remap applied per PIXEL to alpha = o G inside the compositing kernels -- k coincident children at w = 0 then
   * composite exactly like their parent at every pixel, not only at the centre (which of the two the
   * reference's kernel implements is not recoverable from its checkout: gaussian_renderer/__init__.py:258-265 only
   * passes the tensors on).  Must hold the same value in the forward and the backward call. */
  int32_t lod_per_pixel;
  /* Half-precision attribute rows for the in-kernel LOD interpolation (the word that was `reserved1`; 0 = today's
   * behaviour, ABI unchanged).  1, valid only together with lod_render_indices and FORWARD ONLY: shs, opacities, scales
   * and rotations point at arrays of IEEE half ([lod_rows, M, 3], [lod_rows], [lod_rows, 3], [lod_rows, 4] -- the slot
   * arrays hgs_resid_fetch_half_slots fills; shs and rotations 16-byte aligned, as for float32 arrays), means3D
   * stays float32, and the skybox tail rows are read the same way.  The per-Gaussian kernel widens every half exactly
   * as it loads it and then takes the float32 path unchanged -- the weight-1 rule, the separately rounded lerp, the
   * hemisphere flip, the opacity remap -- so the call renders bit for bit what it renders on float32 arrays holding the
   * widened values.  Refused with HGS_ERR_INVALID before any HIP call: by the three forward calls without
   * lod_render_indices, with prepare_backward, with shs_rest / activations / colors_precomp / cov3D_precomp, or with a
   * value other than 0 or 1; by hgs_raster_bwd with any value other than 0. */
  int32_t lod_half_rows;
  /* The caller will run hgs_raster_bwd on the workspaces of this forward (must hold the SAME value in the forward and
   * in the backward call).  The forward's per-Gaussian kernel then also stores, next to the colour, the 3x3 Jacobian
   * d(rgb)/d(view direction) (36 bytes per Gaussian, in geom_ws): it has the SH coefficients in registers anyway, and
   * the backward's SH kernel no longer has to read them again (192 of its 396 bytes per Gaussian at M = 16).
   * 0: nothing extra is stored (inference), the backward recomputes from the coefficients. */
  int32_t prepare_backward;
  /* In-kernel LOD interpolation.  lod_render_indices != NULL: the attribute arrays (means3D,
   * scales, rotations, opacities, shs) hold ALL lod_rows hierarchy Gaussians and row i of the op is
   *     i <  lod_n :  w_i * attr[lod_render_indices[i]] + (1 - w_i) * attr[lod_parent_indices[i]],  w_i = interpolation_weights[i]
   *                   (every product and the sum rounded separately, as the torch expression of
   *                   gaussian_renderer/__init__.py:204-218 rounds; the parent quaternion flipped into the node's hemisphere)
   *     i >= lod_n :  attr[lod_rows - (P - lod_n) + (i - lod_n)]   -- the skybox tail (:220-234)
   * computed in registers by the per-Gaussian kernels of the forward AND of the backward: no interpolated row is ever
   * written to memory.  Needs shs + scales + rotations (no precomputed colours / covariances, no activations),
   * interpolation_weights / num_node_kids with >= P entries, prepare_backward = 1 for a differentiable call.
   * Backward, lod_scatter = 0: the gradients w.r.t. the INTERPOLATED rows ([P, ...]) are written; hgs_lod_gather_bwd
   * scatters them.  lod_scatter = 1 (needs 3M % 4 == 0): the backward's per-Gaussian kernels scatter themselves --
   * grads.dL_dmeans3D / dL_dscales / dL_drotations / dL_dopacity / dL_dshs then point at FULL arrays ([lod_rows, ...],
   * ZERO-FILLED by the caller) and receive w_i * g_i at the node row and the sum of (1 - w_i) * g_i over each run of
   * siblings at the parent row (the parent quaternion's hemisphere flip applied); no row gradient is ever written to
   * memory.  Runs are found among CONSECUTIVE rows (expand_to_size emits non-decreasing parents: every parent is then
   * written once, without atomics, bit-reproducibly); other orders are detected and fall back to atomic adds.
   * dL_dmeans2D stays per row ([P, 3]).  Precondition (as for hgs_lod_gather_bwd): render indices unique, no drawn row is
   * another entry's parent row -- true for any LOD cut. */
  int32_t lod_n;
  const int32_t* lod_render_indices;
  const int32_t* lod_parent_indices;
  int32_t lod_rows;
  int32_t lod_scatter;
} hgs_raster_args;

enum {
  HGS_ACT_SCALE_EXP = 1,       /* scales = exp(raw)                     scene/gaussian_model.py:110 */
  HGS_ACT_ROT_NORMALIZE = 2,   /* rotations = raw / max(|raw|, 1e-12)   scene/gaussian_model.py:114 */
  HGS_ACT_OPACITY_SIGMOID = 4, /* opacities = sigmoid(raw)              scene/gaussian_model.py:126-127 */
  HGS_ACT_OPACITY_ABS = 8      /* opacities = |raw| (hierarchy mode)    scene/gaussian_model.py:393 */
};
/* Activated values are DEFINED as the double-precision result rounded once to float32 (deterministic on every
 * platform); the discrete outputs (radii, tile rectangles, sort keys) follow from those float32 values. */

/* Workspace sizes in bytes.  geom: per-Gaussian state (P); bin: per-instance
 * keys/lists + tile ranges (L = number of (tile,Gaussian) instances, known after
 * stage 1); img: per-pixel state; bwd: backward scratch. */
int hgs_raster_ws_sizes(int32_t P, int32_t width, int32_t height, uint32_t L,
                        size_t* geom_bytes, size_t* bin_bytes, size_t* img_bytes, size_t* bwd_bytes);

/* Stage 1: per-Gaussian preprocess (cull, project, 3D->2D covariance, SH colour,
 * tile rectangle) + offsets scan.  Writes radii[P]; returns L on the host (one
 * 4-byte D2H copy + stream sync -- the only sync of the forward pass). */
int hgs_raster_fwd_stage1(const hgs_raster_args* a, void* geom_ws, int32_t* radii,
                          uint32_t* L_out_host, hgs_stream_t stream, int device);

/* Stage 2: key generation, radix sort by (tile|depth), tile ranges, tile
 * compositing.  out_color [3,H,W], out_invdepth [1,H,W] (may be NULL when
 * !do_depth). */
int hgs_raster_fwd_stage2(const hgs_raster_args* a, void* geom_ws, void* bin_ws, void* img_ws,
                          uint32_t L, float* out_color, float* out_invdepth,
                          hgs_stream_t stream, int device);

/* Single-call forward for callers that can bound L in advance (the Python host uses 1.25 x the previous
 * frame's count): bin_ws / bwd scratch are sized with L_cap, every kernel is enqueued before the host reads
 * L, so the GPU never idles between the stages (the two-stage path leaves a ~50 us bubble).  The call still
 * returns the exact L: the kernel that completes the scans of K1's workgroup sums (K3's last workgroup; the scan launch
 * on the fallback routes) stores it into a pinned, device-mapped host word and the host polls the event
 * recorded behind that kernel (no copy command in the stream; HGS_COUNT_BY_COPY / HGS_BLOCKING_WAIT in the environment
 * select a copy / a sleeping wait instead -- same results).  If L > L_cap it returns HGS_ERR_CAPACITY,
 * the outputs are invalid and the caller continues with hgs_raster_fwd_stage2 on an exactly sized bin_ws
 * (geom_ws / radii from this call stay valid).  Later calls (backward, views) must pass the same L_cap as L.
 * Library state: this entry point keeps, per (device, stream), 40 KB of zeroed device memory between calls (K1 adds its
 * workgroup sums there, a later kernel of the same call clears them; INTEGRATION.md "What the library keeps").  Not for
 * hipStreamPerThread (one handle, one stream per host thread) and not for a capturing stream: both take the scan launch.
 * hgs_release_device_state frees the blocks. */
int hgs_raster_fwd(const hgs_raster_args* a, void* geom_ws, void* bin_ws, void* img_ws, uint32_t L_cap,
                   int32_t* radii, float* out_color, float* out_invdepth, uint32_t* L_out_host,
                   hgs_stream_t stream, int device);

/* Frees what hgs_raster_fwd keeps per (device, stream) for `device` (< 0: every device); returns the number of blocks
 * freed.  No call of the library may be in flight on that device.  The next forward on a stream creates its block again. */
int hgs_release_device_state(int device);

typedef struct hgs_raster_grads {
  float* dL_dmeans3D;   /* [P,3] */
  float* dL_dmeans2D;   /* [P,3]  gradient w.r.t. NDC-scaled screen position (consumer: scene/gaussian_model.py:687-689) */
  float* dL_dshs;       /* [P,M,3] or NULL */
  float* dL_dcolors;    /* [P,3]  or NULL */
  float* dL_dopacity;   /* [P] */
  float* dL_dscales;    /* [P,3] or NULL */
  float* dL_drotations; /* [P,4] or NULL */
  float* dL_dcov3D;     /* [P,6] or NULL */
  float* dL_dshs_rest;  /* [P,M-1,3] with args.shs_rest (dL_dshs is then [P,1,3]), else NULL */
} hgs_raster_grads;

/* Backward.  Needs the forward outputs (out_color, out_invdepth) and the
 * workspaces exactly as stage 2 left them.  dL_dinvdepth may be NULL. */
int hgs_raster_bwd(const hgs_raster_args* a, const void* geom_ws, const void* bin_ws,
                   const void* img_ws, void* bwd_ws, uint32_t L,
                   const float* out_color, const float* out_invdepth,
                   const float* dL_dcolor, const float* dL_dinvdepth,
                   const hgs_raster_grads* grads, hgs_stream_t stream, int device);

/* Per-Gaussian blending statistics of ONE forward whose workspaces are intact: for every
 * row i < P of the op that the forward blended into at least one counted pixel, with s = slot_of_row[i],
 *     wmax[s]  = max(wmax[s], largest w = alpha * T_before over the counted pixels)     float32
 *     wsum[s] += sum of w over the counted pixels                                        float64
 *     count[s] += number of counted pixels the row is blended at                         int64
 * and every other entry of the three [n_slots] device arrays keeps its bits: zero-fill once, call once per view.
 * "Blended" is K6's decision on the same records in the same float32 expressions (list membership, exponent clamped
 * at 0, alpha = min(0.99, o G) >= 1/255, pixel not stopped, T after it >= 1e-4); o is the opacity K1 stored, so the
 * default per-Gaussian LOD remap is included.  Stands in for nothing upstream; in this library it replaces the
 * colour-gradient trick (render with colors_precomp, back-propagate ones through hgs_raster_bwd, read one channel of
 * dL_dcolors), which yields wsum alone at the cost of the whole backward.
 *   pixel_mask   NULL (all pixels) or device uint8 [H*W], non-zero = counted
 *   slot_of_row  NULL (identity; then n_slots >= P) or device int32 [P]; a negative entry ignores the row, and so does
 *                an entry >= n_slots (bounded in the kernel: never written through).  PRECONDITION: the entries in
 *                [0, n_slots) are distinct (true of the render_indices of any LOD cut) -- slots are updated with plain
 *                read-modify-writes.
 *   tmp          hgs_raster_contrib_tmp_bytes(L) bytes of device scratch, uninitialised; L as for hgs_raster_bwd (the
 *                L_cap of a single-call forward; a forward that returned HGS_ERR_CAPACITY must have been completed by
 *                stage 2 first).
 * Asynchronous on `stream`, no host wait, no atomics: the same inputs give the same bits on every run.  L == 0 or
 * P == 0 returns HGS_OK and writes nothing.  Refused with HGS_ERR_INVALID before any HIP call (hgs_last_error names
 * it): what the forward's argument check refuses, lod_per_pixel != 0 (not built), a null output, n_slots < 1,
 * n_slots < P without slot_of_row, a null workspace or tmp.  lod_half_rows is ALLOWED: the call reads the float32
 * records, lists and offsets of the forward and none of its attribute rows. */
size_t hgs_raster_contrib_tmp_bytes(uint32_t L);
int hgs_raster_contrib(const hgs_raster_args* a, const void* geom_ws, const void* bin_ws, const void* img_ws,
                       uint32_t L, const uint8_t* pixel_mask, const int32_t* slot_of_row, int64_t n_slots,
                       float* wmax, double* wsum, int64_t* count, void* tmp, hgs_stream_t stream, int device);

/* A per-pixel image attributed to the Gaussians that blend it, on ONE forward whose workspaces are intact (DESIGN.md
 * section 7, f-23): for every row i < P of the op that the forward blended into at least one counted pixel, with
 * s = slot_of_row[i],
 *     out[s * channels + c] += sum over the counted pixels p the row is blended at of  w(p) * image[c][p]      float64
 *     wsum[s]               += sum of w over the same pixels (when wsum is given)                            float64
 * with w = alpha * T_before exactly as hgs_raster_contrib states it ("blended" is K6's decision on the same records in
 * the same float32 expressions), and every other entry keeps its bits: zero-fill once, call once per view.  wsum
 * equals hgs_raster_contrib's bit for bit, and so does a channel of ones.  w * image is one rounded float32 product per
 * pixel; a pixel that is not counted, or at which the row is not blended, contributes a selected zero and its image value
 * is not multiplied in (masked-out and outside pixels are not read at all): a NaN or infinity there reaches no output.
 * Stands in for nothing upstream; in this library it replaces dL / d colors_precomp of hgs_raster_bwd seeded with the
 * image -- the whole backward, refused on the in-op LOD route and without a slot map.
 *   image        device float32, planar [channels, H, W] (the layout the rasterizer returns); channels in 1..3
 *   pixel_mask   NULL (all pixels) or device uint8 [H*W], non-zero = counted
 *   slot_of_row  NULL (identity; then n_slots >= P) or device int32 [P]; a negative entry ignores the row, and so does
 *                an entry >= n_slots (bounded in the kernel: never written through).  PRECONDITION: the entries in
 *                [0, n_slots) are distinct -- slots are updated with plain read-modify-writes.
 *   out          device float64 [n_slots, channels];  wsum: device float64 [n_slots] or NULL
 *   tmp          hgs_raster_attribute_tmp_bytes(L) bytes of device scratch, uninitialised; L as for hgs_raster_contrib.
 * Asynchronous on `stream`, no host wait, no atomics: the same inputs give the same bits on every run.  L == 0 or
 * P == 0 returns HGS_OK and writes nothing.  Refused with HGS_ERR_INVALID before any HIP call (hgs_last_error names
 * it): everything hgs_raster_contrib refuses (the forward's argument check, lod_per_pixel != 0, n_slots < 1,
 * n_slots < P without slot_of_row, a null workspace or tmp), channels outside 1..3, a null image, a null out.
 * lod_half_rows is ALLOWED: none of the forward's attribute rows is read. */
size_t hgs_raster_attribute_tmp_bytes(uint32_t L);
int hgs_raster_attribute(const hgs_raster_args* a, const void* geom_ws, const void* bin_ws, const void* img_ws,
                         uint32_t L, const float* image, int32_t channels, const uint8_t* pixel_mask,
                         const int32_t* slot_of_row, int64_t n_slots, double* out /* [n_slots, channels] */,
                         double* wsum /* [n_slots] or NULL */, void* tmp, hgs_stream_t stream, int device);

/* Per-pixel readout of ONE forward whose workspaces are intact: what a pixel shows.  For
 * every pixel p inside the image take the rows K6 blended there, front to back, k = 1..n ("blended" is K6's decision on
 * the same records in the same float32 expressions, as hgs_raster_contrib states it), with w_k = alpha_k * T_{k-1} and
 * T_k as K6 computes them.  Each plane is a device array [H*W] or NULL; at least one must be given.
 *     alpha         float32  1.0f - T_n (one float32 subtraction; the bits of 1 - final_T); 0 where n = 0
 *     count         int32    n
 *     front, back   int32    id of row k = 1 / k = n
 *     heaviest      int32    id of the row with the largest w_k, the front-most one on equal bits;  wmax: that weight
 *     median        int32    id of the first k with T_k < 0.5f;  median_depth: the view-space depth K1 stored for that
 *                            row (bits copied); no such k: id -1, depth 0
 * The id of op row i is slot_of_row[i] when that lies in [0, n_slots), i itself when slot_of_row is NULL, and -2 when
 * the map ignores the row (negative or >= n_slots): an ignored row still occludes and counts in `count` and `alpha`, it
 * only cannot be named.  Where there is no row the id is -1, wmax 0 and median_depth 0.  Every pixel inside the image is
 * written in every given plane: the caller need not pre-fill.
 * One launch, asynchronous on `stream`, no host wait, no atomics, no scratch: the same inputs give the same bits on
 * every run.  L == 0 or P == 0 fills the planes with the "nothing" values (no workspace is read then).  Refused with
 * HGS_ERR_INVALID before any HIP call (hgs_last_error names it): what the forward's argument check refuses,
 * lod_per_pixel != 0 (not built), all planes NULL, a null workspace, n_slots < 1 with a map.  lod_half_rows and the
 * in-op LOD route are ALLOWED: only records, lists, ranges and depths are read. */
typedef struct {
  float* alpha;
  int32_t* count;
  int32_t* front;
  int32_t* back;
  int32_t* heaviest;
  float* wmax;
  int32_t* median;
  float* median_depth;
} hgs_raster_pixel_planes;
int hgs_raster_pixels(const hgs_raster_args* a, const void* geom_ws, const void* bin_ws, const void* img_ws, uint32_t L,
                      const int32_t* slot_of_row, int64_t n_slots, const hgs_raster_pixel_planes* out,
                      hgs_stream_t stream, int device);

/* Per-row values painted into the picture of ONE forward whose workspaces are intact: the
 * dual of hgs_raster_attribute.  For every pixel p inside the image take the rows K6 blended there, front to back,
 * k = 1..n ("blended" is K6's decision on the same records in the same float32 expressions, as hgs_raster_contrib
 * states it), with w_k = alpha_k * T_{k-1} and T_n as K6 computes them, and with s_k the slot of row k:
 *     out[c][p] = fma(T_n, background[c], acc_n),   acc_k = fma(w_k, values[s_k * value_stride + c], acc_{k-1}),  acc_0 = 0
 *     wsum[p]   = sum over the NAMED rows, in the same order, of w_k                     (float32; when wsum is given)
 * all float32, one fused multiply-add per row, in list order: with finite values these are the bits K6 gives a colour
 * channel whose per-row colours are `values` (and, with a NULL background, its inverse-depth plane).  A row that is not
 * blended at p is SKIPPED, not weighted by zero: a NaN or an infinity in a row's values reaches exactly the pixels the
 * row is blended at.  The slot of op row i is slot_of_row[i] when that lies in [0, n_slots) -- the row is then NAMED --
 * and i itself when slot_of_row is NULL; a row the map ignores (negative or >= n_slots) still occludes, its values are
 * never read, and it adds nothing to out or wsum.  Stands in for nothing upstream; in this library it replaces a second
 * whole forward with colors_precomp (K1, binning and sort again, three channels, no slot map).
 *   values       device float32 [n_slots, value_stride], read at the first `channels` words of a row;  channels in 1..4,
 *                value_stride >= channels (wider tables go through in groups of four by offsetting `values`)
 *   slot_of_row  NULL (identity; then n_slots >= P) or device int32 [P] (the render_indices of a cut: values per node)
 *   background   NULL (zeros: the stored bits are acc_n's) or device float32 [channels]
 *   out          device float32, planar [channels, H, W];  wsum: device float32 [H*W] or NULL
 * Every pixel inside the image is written in every given plane: the caller need not pre-fill.  One launch, asynchronous
 * on `stream`, no host wait, no atomics, no scratch: the same inputs give the same bits on every run.  L == 0 or P == 0
 * reads no workspace and no value: out takes the background and wsum zeros.  Refused with HGS_ERR_INVALID before any HIP
 * call (hgs_last_error names it): what the forward's argument check refuses, lod_per_pixel != 0 (not built), channels
 * outside 1..4, value_stride < channels, null values or out, n_slots < 1, n_slots < P without slot_of_row, a null
 * workspace.  lod_half_rows and the in-op LOD route are ALLOWED: only records, lists and ranges are read. */
int hgs_raster_values(const hgs_raster_args* a, const void* geom_ws, const void* bin_ws, const void* img_ws, uint32_t L,
                      const float* values, int64_t value_stride, int channels /* 1..4 */,
                      const int32_t* slot_of_row, int64_t n_slots, const float* background /* [channels] or NULL */,
                      float* out /* [channels, H, W] */, float* wsum /* [H*W] or NULL */, hgs_stream_t stream, int device);

/* SH part of the backward for up to HGS_MAX_DEFERRED_VIEWS views of the SAME Gaussians in one pass (gradient
 * accumulation over the views of one optimiser step / of one data-parallel rank): the [P,M,3] coefficients are read
 * once and dL_dshs is written once, instead of once per view.  Each view ran hgs_raster_bwd with
 * args.defer_sh_bwd = 1; its geom_ws and bwd_ws (the per-Gaussian colour gradients live there) must still be intact.
 * dL_dshs = (accumulate ? dL_dshs : 0) + sum over the views; dL_dmeans3D += the views' view-direction terms. */
#define HGS_MAX_DEFERRED_VIEWS 8
typedef struct hgs_sh_bwd_view {
  const void* geom_ws;
  const void* bwd_ws;
  const float* campos; /* device [3] */
  uint32_t L;          /* the L the view's hgs_raster_bwd was called with */
  uint32_t reserved;
} hgs_sh_bwd_view;
int hgs_raster_sh_bwd_batched(const hgs_sh_bwd_view* views, int32_t n_views, int32_t P, int32_t M, int32_t sh_degree,
                              const float* means3D, const float* shs, float* dL_dshs, float* dL_dmeans3D,
                              int32_t accumulate, hgs_stream_t stream, int device);

/* View-dependent colours of the same Gaussians for up to HGS_MAX_DEFERRED_VIEWS cameras in one pass over the SH
 * coefficients -- the batched HIP form of the reference's convert_SHs_python branch (gaussian_renderer/__init__.py:
 * 84-89: eval_sh + 0.5, clamped at 0, result handed to the rasterizer as colors_precomp).  Forward writes rgb [P,3] and
 * a clamp mask [P] (bit c set: channel c was clamped) per view; backward takes dL/d(rgb) per view (the dL_dcolors of
 * the views' hgs_raster_bwd), masks it, and writes dL_dshs = (accumulate ? dL_dshs : 0) + sum over the views and
 * dL_dmeans3D += the view-direction terms. */
typedef struct hgs_sh_color_view {
  const float* campos;  /* device [3] */
  float* rgb;           /* forward out [P,3] */
  uint8_t* clamp;       /* forward out / backward in [P] */
  const float* d_rgb;   /* backward in [P,3] */
} hgs_sh_color_view;
int hgs_sh_colors_batched(const hgs_sh_color_view* views, int32_t n_views, int32_t P, int32_t M, int32_t sh_degree,
                          const float* means3D, const float* shs, hgs_stream_t stream, int device);
int hgs_sh_colors_batched_bwd(const hgs_sh_color_view* views, int32_t n_views, int32_t P, int32_t M, int32_t sh_degree,
                              const float* means3D, const float* shs, float* dL_dshs, float* dL_dmeans3D,
                              int32_t accumulate, hgs_stream_t stream, int device);

/* Introspection for the parity tests ("bit-exact on tile/sort indices"):
 * device pointers into the workspaces after stage 2. */
typedef struct hgs_raster_views {
  const uint32_t* tile_ids_sorted; /* [L] tile id per sorted instance; with depths[point_list[i]] this is the
                                     (tile<<32 | depth bits) key sequence of the reference's sort.  Written by a forward
                                     with args.debug != 0 (and on the radix path of tile grids above 32 768 tiles); the
                                     binning path does not need the column -- entry i lies in [ranges[t][0], ranges[t][1])
                                     of its tile t, which is how the Python host rebuilds it */
  const uint32_t* point_list;    /* [L] Gaussian id per sorted instance */
  const uint32_t* ranges;        /* [T,2] start,end per tile */
  const uint32_t* tiles_touched; /* [P] */
  const uint32_t* offsets;       /* [P] exclusive scan of tiles_touched */
  const float* depths;           /* [P] view-space z */
  const uint32_t* rects;         /* [P,2] packed (x | y<<16) min, max in tile units */
  const float* records;          /* [P,16] per-Gaussian 2D record, 64 bytes */
  const float* final_T;          /* [H*W] */
  const uint32_t* n_contrib;     /* [H*W] */
} hgs_raster_views;
int hgs_raster_views_get(int32_t P, int32_t width, int32_t height, uint32_t L, const void* geom_ws,
                         const void* bin_ws, const void* img_ws, hgs_raster_views* out);

/* Standalone device sort of (u64 key, u32 value) pairs, stable, LSD radix over
 * bits [0, end_bit).  Exposed for the sort parity tests.  tmp_bytes from
 * hgs_sort_tmp_bytes. Result lands in keys_out/vals_out. */
size_t hgs_sort_tmp_bytes(uint32_t n);
int hgs_sort_pairs(const uint64_t* keys_in, const uint32_t* vals_in, uint64_t* keys_out,
                   uint32_t* vals_out, void* tmp, uint32_t n, int end_bit,
                   hgs_stream_t stream, int device);

/* Optional per-stage timing with hipEvents recorded on the caller's stream (bench.py's
 * per-kernel roofline figures).  Off by default; no reference counterpart (the reference
 * records CUDA events it never reads: train_single.py:41-42,86,124). */
/* on: 0 = off, 1 = every stage, otherwise a mask with bit (1 + i) selecting stage i only (two events per timed
 * stage are recorded on the stream, so timing one kernel perturbs a measured region less than timing all). */
int hgs_timing_enable(int on);
int hgs_timing_stage_count(void);
const char* hgs_timing_stage_name(int i);
/* Resolves all pending events (blocks until they completed) and returns the accumulated
 * milliseconds and call counts per stage; reset != 0 clears the accumulators. */
int hgs_timing_read(double* ms_out, uint32_t* calls_out, int reset);

/* ---------------------------------------------------------------------------
 * Hierarchy LOD cut.  Replaces gaussian_hierarchy._C.expand_to_size and
 * get_interpolation_weights (train_post.py:91-113, render_hierarchy.py:58-80).
 *   nodes int32 [N,7] = depth,parent,start,count_leafs,count_merged,start_children,count_children
 *   boxes f32  [N,2,4] = min.xyz + extent, max.xyz + pad
 * size(n, v) = extent(n) / dist(v, AABB(n)), FLT_MAX for v inside the box.
 * Cut (top-down from the root): a reached node with size >= tau is too coarse -- its count_leafs own Gaussians
 * [start, start + count_leafs) are drawn and its children are reached; a reached node with size < tau is drawn as
 * a whole (count_leafs + count_merged Gaussians from start).  parent index = nodes[parent].start (own index at the
 * root).  Output in ascending node order.
 * Weight of a cut node: 1 at the root; else with p = min(size(parent), 2 tau), s0 = max(p / 2, size(n)):
 * t = 1 if p <= s0, else max(1 - max(0, tau - s0) / (p - s0), 0); num_siblings = count_children of the parent.
 * ------------------------------------------------------------------------- */
size_t hgs_expand_tmp_bytes(int32_t N);
/* Fills render_indices / parent_indices / nodes_for_render_indices (device, capacity
 * `capacity` entries) and returns the number of entries in *count_out_host (host sync). */
int hgs_expand_to_size(const int32_t* nodes, const float* boxes, int32_t N, float size,
                       const float viewpoint[3], const float viewdir[3],
                       int32_t* render_indices, int32_t* parent_indices,
                       int32_t* nodes_for_render_indices, int32_t capacity, void* tmp,
                       int32_t* count_out_host, hgs_stream_t stream, int device);
/* Same cut in ONE pass over the nodes instead of one launch per tree level -- valid when the boxes NEST (every
 * child's AABB inside its parent's, child extent <= parent extent): then size(parent) >= size(child) from every
 * viewpoint and a node only has to look at its parent.  hgs_hier_boxes_nested checks the precondition (view
 * independent: once per hierarchy; tmp >= 4 bytes of device memory); the Python binding caches the answer per
 * (nodes, boxes) pair and falls back to hgs_expand_to_size when it is 0.  Same arguments, same outputs. */
int hgs_expand_to_size_nested(const int32_t* nodes, const float* boxes, int32_t N, float size,
                              const float viewpoint[3], const float viewdir[3],
                              int32_t* render_indices, int32_t* parent_indices,
                              int32_t* nodes_for_render_indices, int32_t capacity, void* tmp,
                              int32_t* count_out_host, hgs_stream_t stream, int device);
int hgs_hier_boxes_nested(const int32_t* nodes, const float* boxes, int32_t N, void* tmp, int32_t* nested_out_host,
                          hgs_stream_t stream, int device);
int hgs_interp_weights(const int32_t* node_indices, int32_t n, float size, const int32_t* nodes,
                       const float* boxes, int32_t N, const float viewpoint[3], const float viewdir[3],
                       float* interpolation_weights, int32_t* num_siblings,
                       hgs_stream_t stream, int device);

/* ---------------------------------------------------------------------------
 * Frustum-culled cut (ABI 11; opt-in: the calls above are unchanged).  The cut above, minus the entries that a view
 * cannot draw, with the weights and sibling counts of the kept entries, in one call.
 *   Bound of node n: a ball (c_n, R_n) around its own rows [start, start + count_leafs + count_merged): c_n = the mean
 *   of the rows' means, R_n = max_i(|m_i - c_n| + 3 max_k s_i,k) on ACTIVATED scales; bounds f32 [N,4] = (c, R); a node
 *   without rows gets R = +inf.  View independent: rebuilt only when the rows change (one launch).
 *   Planes: f32 [5,4] HOST values, rows (a, d) with |a| = 1 and a.x + d >= 0 inside: the four side planes through the
 *   camera centre at tangents fov_scale * tanfov, fov_scale = max(1.3, 1 + 36 / min(W, H)) (1.3: the rasterizer's clamp
 *   on t.x / t.z), and the near plane view z = 0.2 (the rasterizer's cull).
 *   radius_scale = max(1, scale_modifier) * sqrt((1 + 1.69 (tx^2 + ty^2)) / (1 + 1.69 min(tx, ty)^2)), tx, ty = tanfov.
 *   Cull: an entry of node n with parent p (the root: p = n) is dropped iff for some plane k BOTH
 *   a_k.c_n + d_k + radius_scale R_n < 0 and a_k.c_p + d_k + radius_scale R_p < 0 (float32, left to right, no
 *   contraction).  The weight plays no part.  The kept entries keep their order, parents, weights, sibling counts.
 * ------------------------------------------------------------------------- */
/* bounds[N,4] from the node list and the [G,3] means / activated scales (device).  A node whose rows leave [0, G) is an
 * error (HGS_ERR_INVALID, the node is named); host sync.  The word that check reports through is allocated and freed
 * inside the call (4 bytes; a bounds build happens once per hierarchy), so the call takes no workspace. */
int hgs_hier_cull_bounds(const int32_t* nodes, int32_t N, const float* means, const float* scales, int32_t G,
                         float* bounds, hgs_stream_t stream, int device);
size_t hgs_lod_cut_view_tmp_bytes(int32_t N);
/* nested != 0: the single-pass route (precondition: hgs_hier_boxes_nested), else level by level.  The five outputs hold
 * `capacity` entries each; *count_out_host = kept entries, *unculled_out_host = what hgs_expand_to_size would have
 * returned (one host sync).  More kept entries than `capacity`: HGS_ERR_INVALID, the message and *count_out_host give
 * the count, nothing is written past the capacity.  N <= 0: no entries, no GPU work. */
int hgs_lod_cut_view(const int32_t* nodes, const float* boxes, const float* bounds, int32_t N, float size,
                     const float viewpoint[3], const float planes[20], float radius_scale, int32_t nested,
                     int32_t* render_indices, int32_t* parent_indices, int32_t* nodes_for_render_indices,
                     float* weights, int32_t* num_siblings, int32_t capacity, void* tmp, int32_t* count_out_host,
                     int32_t* unculled_out_host, hgs_stream_t stream, int device);

/* ---------------------------------------------------------------------------
 * Budget-exact cut (ABI 12; opt-in: the calls above are unchanged).  The finest
 * granularity tau* >= tau_min whose cut costs at most `budget`, and the cut at tau* -- exactly what hgs_lod_cut_view
 * returns at tau*: entries, order, parents, weights, sibling counts, bit for bit -- in one call with one host wait.
 * Precondition: the boxes NEST (hgs_hier_boxes_nested); the cost of the cut at tau is then a sum of indicator functions.
 * With s_n = size(n, v), s_par the parent's (+inf at the root), L / M = count_leafs / count_merged and k_n = 1 unless the
 * cull above drops the entry of n (planes == NULL: k_n = 1):
 *   HGS_CUT_COST_ENTRIES  entries(tau) = sum_n k_n ([s_par >= tau] (L + M) - [s_n >= tau] M)
 *   HGS_CUT_COST_ROWS     rows(tau) = entries(tau) + #{p : s_p / 2 < tau <= s_p and m_p < tau}, m_p = the smallest s_c
 *                         over p's children c with k_c = 1 and L_c + M_c > 0: the entries plus the distinct parent rows
 *                         that entries of weight < 1 read (the weight is 1 whenever s_p >= 2 tau) = the rows
 *                         hgs_resid_mark needs when no node with children owns leaf rows (else an upper bound).
 * Every comparison is on the float32 sizes as size() gives them; s_p / 2 is exact (sizes are not subnormal in practice).
 * Write cost(t) for the cost at the tau whose bit pattern is t (non-negative floats order as their bit patterns).
 *   cost(tau_min) <= budget: tau* = tau_min (the request fits).
 *   Else a radix descent over t with the invariant cost(lo) > budget >= cost(hi), from lo = bits(tau_min),
 *   hi = bits(+inf) (cost: the root's kept rows), in THREE digits of 11, 10 and 10 bits (steps 2^20, 2^10, 1): at each
 *   digit the cost is evaluated at the multiples of the step inside (lo, hi] (hi is one of them), lo moves to the
 *   highest one whose cost exceeds the budget (stays if none does) and hi to the next one above it; after the last
 *   digit hi = lo + 1 and tau* = hi.  So cost(tau*) <= budget < cost(prev(tau*)): tau* is locally tight, and the
 *   smallest fitting granularity wherever the cost does not increase with tau (always for ENTRIES without planes).
 *   budget < cost(+inf): HGS_ERR_CAPACITY, the message and *cost_out_host give the count, no output is written.
 * bounds and planes are both given or both NULL.  The five outputs hold `capacity` >= budget entries each.  NULL
 * pointers, N <= 0, budget < 0, a negative or NaN tau_min, an unknown cost_mode and capacity < budget are refused before
 * any HIP call.  Node records that point outside the list, sizes that are negative or NaN and (ROWS) a child larger
 * than its parent from this viewpoint: HGS_ERR_INVALID, no output is written.  All sums are integer: two calls give
 * the same bits.  *count_out_host = kept entries, *unculled_out_host = entries of the unculled cut at tau*.
 * ------------------------------------------------------------------------- */
#define HGS_CUT_COST_ENTRIES 0
#define HGS_CUT_COST_ROWS 1
size_t hgs_lod_cut_budget_tmp_bytes(int32_t N);
int hgs_lod_cut_budget(const int32_t* nodes, const float* boxes, const float* bounds, int32_t N, float tau_min,
                       int32_t budget, int32_t cost_mode, const float viewpoint[3], const float planes[20],
                       float radius_scale, int32_t* render_indices, int32_t* parent_indices,
                       int32_t* nodes_for_render_indices, float* weights, int32_t* num_siblings, int32_t capacity,
                       void* tmp, int32_t* count_out_host, int32_t* unculled_out_host, float* tau_out_host,
                       int32_t* cost_out_host, hgs_stream_t stream, int device);

/* ---------------------------------------------------------------------------
 * Cut for several views (opt-in: the calls above are unchanged).  What
 * hgs_lod_cut_view gives for each of V <= HGS_CUT_MAX_VIEWS views (granularity sizes[v], viewpoint, five planes and
 * radius scale of its own) -- entries, order, parents, weights, sibling counts, bit for bit -- from ONE pass over the
 * nodes and one host wait: a node's record, boxes and ball are loaded once and judged for every view.
 * Precondition: the boxes NEST (hgs_hier_boxes_nested); only the single-pass route exists.
 * bounds and planes are both given (planes f32 [V,5,4] HOST values) or both NULL: then nothing is culled and view v gets
 * hgs_expand_to_size + hgs_interp_weights, unculled_out_host[v] = counts_out_host[v].
 * The five outputs hold `capacity` entries each and are PACKED: the n_v = counts_out_host[v] entries of view v start at
 * offsets_out_host[v] = sum over u < v of roundup4(n_u), so every view's slice starts on 16 bytes; the up to 3 entries
 * between two views are not written.  *needed_out_host = offsets[V - 1] + n_{V - 1}.  needed > capacity: HGS_ERR_INVALID,
 * the message names the needed count, counts / offsets / needed are set and nothing at or past `capacity` was written
 * (positions are 64-bit).  needed > 2^31 - 1: refused, the message says so (counts and offsets saturate).
 * NULL pointers, V outside [1, HGS_CUT_MAX_VIEWS], capacity < 0 and bounds without planes (or the reverse) are refused
 * before any HIP call.  N <= 0: all counts 0, no GPU work.
 * ------------------------------------------------------------------------- */
#define HGS_CUT_MAX_VIEWS 16
size_t hgs_lod_cut_views_tmp_bytes(int32_t N, int32_t V);
int hgs_lod_cut_views(const int32_t* nodes, const float* boxes, const float* bounds, int32_t N, int32_t V,
                      const float* sizes, const float* viewpoints, const float* planes, const float* radius_scales,
                      int32_t* render_indices, int32_t* parent_indices, int32_t* nodes_for_render_indices,
                      float* weights, int32_t* num_siblings, int32_t capacity, void* tmp, int32_t* counts_out_host,
                      int32_t* unculled_out_host, int32_t* offsets_out_host, int64_t* needed_out_host,
                      hgs_stream_t stream, int device);

/* In-op LOD attribute interpolation: the gather + lerp that render_post does in Python
 * (gaussian_renderer/__init__.py:199-218), for callers that pass GaussianRasterizationSettings.render_indices /
 * parent_indices non-empty.  out_i = w_i * attr[render_indices[i]] + (1 - w_i) * attr[parent_indices[i]]; rotations
 * with the parent quaternion flipped into the node's hemisphere.  Any attribute pointer may be NULL (skipped).
 * Every product and the sum are rounded separately and BOTH rows are always read, exactly as the torch expression: a
 * weight of exactly 1 still multiplies the parent row by 0, so a non-finite parent attribute gives a non-finite row
 * (0 * NaN is NaN).  The weight-1 rule of the in-kernel interpolation (hgs_raster_args.lod_render_indices; stated at
 * lod_row_gather in csrc/gaussian_math.h: the parent of a weight-1 row is not read) does NOT hold for this call. */
int hgs_lod_gather(const int32_t* render_indices, const int32_t* parent_indices, const float* weights, int32_t n,
                   int32_t M, const float* means3D, const float* scales, const float* rotations, const float* shs,
                   const float* opacities, float* o_means3D, float* o_scales, float* o_rotations, float* o_shs,
                   float* o_opacities, hgs_stream_t stream, int device);
/* Backward: g_* = gradients of the n interpolated rows; d_* = gradients of the full arrays, ZERO-INITIALISED by
 * the caller; rotations = the full forward input (sign of the hemisphere flip); flag_tmp = 4 bytes of device
 * scratch.  Precondition: render_indices are unique and no rendered row is another entry's parent row (true for
 * any LOD cut). */
int hgs_lod_gather_bwd(const int32_t* render_indices, const int32_t* parent_indices, const float* weights, int32_t n,
                       int32_t M, const float* rotations, const float* g_means3D, const float* g_scales,
                       const float* g_rotations, const float* g_shs, const float* g_opacities, float* d_means3D,
                       float* d_scales, float* d_rotations, float* d_shs, float* d_opacities, uint32_t* flag_tmp,
                       hgs_stream_t stream, int device);

/* ---------------------------------------------------------------------------
 * Fused row-sparse Adam.  Replaces the gather / update / scatter chain of
 * scene/OurAdam.py:249-337 (_single_tensor_adam; dense variant :339-420) for ALL parameter tensors of the model in
 * one launch.  Every tensor is [P, row_len] contiguous f32; bias corrections and step size are computed by the caller
 * (step_size = lr / (1 - beta1^t), bias_correction2_sqrt = sqrt(1 - beta2^t), as the Python code does in double).
 * rows != NULL: update the n_rows listed rows (int64, as `relevant` in train_single.py:171-174);
 * row_mask_grad != NULL: update row r iff row_mask_grad[r] != 0 (the same selection, evaluated in-kernel);
 * both NULL: dense update of all P rows.
 * ------------------------------------------------------------------------- */
#define HGS_ADAM_MAX_TENSORS 8
typedef struct hgs_adam_tensor {
  float* param;
  const float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  int32_t row_len;
  float step_size;
  float beta1, one_minus_beta1; /* both rounded from double by the caller, as torch does with its scalar arguments */
  float beta2, one_minus_beta2;
  float eps, weight_decay;
  float bias_correction2_sqrt;
  int32_t reserved;
} hgs_adam_tensor;
int hgs_adam_step(const hgs_adam_tensor* tensors, int32_t n_tensors, int64_t P, const int64_t* rows, int64_t n_rows,
                  const float* row_mask_grad, hgs_stream_t stream, int device);

/* ---------------------------------------------------------------------------
 * simple_knn._C.distCUDA2 (scene/gaussian_model.py:190): mean squared distance
 * to the 3 nearest neighbours.  tmp_bytes from hgs_knn_tmp_bytes.
 * ------------------------------------------------------------------------- */
size_t hgs_knn_tmp_bytes(int32_t P);
int hgs_dist2_knn3(const float* xyz, int32_t P, float* out_mean_d2, void* tmp,
                   hgs_stream_t stream, int device);

/* ---------------------------------------------------------------------------
 * .hier files.  Replaces gaussian_hierarchy._C.load_hierarchy / write_hierarchy
 * (scene/gaussian_model.py:329,420-427).  Host memory only.
 * ------------------------------------------------------------------------- */
enum {
  HGS_HIER_UPSTREAM = 0,      /* header-less layout of the gaussian-hierarchy tools: int P, pos, rot, log-scale, alpha,
                               * sh[16][3], int N, nodes, boxes (restated from the public repository; see hier_io.cpp) */
  HGS_HIER_PRIVATE = 1,       /* "HGSHIER1" + P, N, M: any SH count */
  HGS_HIER_UPSTREAM_HALF = 2  /* upstream layout with P < 0 (the file stores -P): rot / log-scale / alpha / sh stored as
                               * IEEE half under the narrowing rule of HGS_RESID_HOST_ROW_BYTES_HALF below, positions
                               * float32: 124 bytes per Gaussian instead of 236.  M = 16 only */
};
typedef struct hgs_hier_host {
  int32_t P;      /* Gaussians */
  int32_t N;      /* nodes */
  int32_t M;      /* SH coefficients per Gaussian (16) */
  int32_t reserved; /* layout: one of the HGS_HIER_* above for hgs_hier_write; hgs_hier_load reports what it found */
  float* xyz;         /* [P,3] */
  float* shs;         /* [P,M,3] */
  float* alpha;       /* [P] activated opacity */
  float* log_scales;  /* [P,3] */
  float* rots;        /* [P,4] */
  int32_t* nodes;     /* [N,7] */
  float* boxes;       /* [N,2,4] */
} hgs_hier_host;
int hgs_hier_load(const char* path, hgs_hier_host* out); /* allocates; release with hgs_hier_free */
int hgs_hier_write(const char* path, const hgs_hier_host* in);
void hgs_hier_free(hgs_hier_host* h);

/* ---------------------------------------------------------------------------
 * Hierarchy construction on the device: the rule of hgs.hierarchy.build_hierarchy.
 * Inputs (device, activated): xyz [P,3], scales [P,3] linear, rots [P,4] (w,x,y,z), opacity [P] in [0,1],
 * shs [P,M,3] with M in {1,4,9,16}; 1 <= P <= 2^30.  Outputs (device) for N = 2P - 1 nodes, Gaussian index == node
 * index, BFS numbering with contiguous children: xyz [N,3], shs [N,16,3] (zero-padded), alpha [N], log_scales [N,3],
 * rots [N,4], nodes int32 [N,7], boxes [N,2,4]; out_shs / out_rots / out_boxes 16-byte aligned.  Leaves keep their
 * input rotation and log of their input scales; interior nodes hold the w = alpha * s0 * s1 * s2 weighted moment match
 * of their children, rotation and scales from an eigen-solve of the merged covariance.  nodes, boxes and the leaf rows
 * of xyz / shs / alpha / rots equal build_hierarchy's bit for bit.
 * hgs_hier_build_tmp_bytes: host only (no GPU needed); 0 for a P outside [1, 2^30].
 * hgs_hier_build: asynchronous on `stream` (level sizes are host arithmetic: no host round trip); sizes are checked
 * before any HIP call. */
size_t hgs_hier_build_tmp_bytes(int32_t P);
int hgs_hier_build(const float* xyz, const float* scales, const float* rots, const float* opacity, const float* shs,
                   int32_t P, int32_t M, float* out_xyz, float* out_shs, float* out_alpha, float* out_log_scales,
                   float* out_rots, int32_t* out_nodes, float* out_boxes, void* tmp, hgs_stream_t stream, int device);

/* ---------------------------------------------------------------------------
 * Consolidation of chunk hierarchies on the device: the rule of hgs.hierarchy.merge_hierarchies applied to chunks
 * trimmed to their first N rows (replaces the upstream GaussianHierarchyMerger call of
 * scripts/full_train.py:240-250).  For k chunks the merged hierarchy has 1 + k + sum(N_c - 1) nodes, one row per node:
 * node 0 is a new root whose children are the chunk roots 1..k; chunk c's node 0 lands at 1 + c and its nodes 1..N_c-1
 * at base_c .. base_c + N_c - 2, with base_0 = 1 + k and base_{c+1} = base_c + N_c - 1.  Depths grow by 1; parent,
 * start and start_children are remapped; rows and boxes are copied unchanged.  Rows at index >= N of a chunk (G > N:
 * the skybox tail train_post.py's save_hier appends) are dropped.
 * hgs_hier_merge_place: copies chunk `index`'s rows and boxes into place (hipMemcpyAsync: the chunk's attribute and box
 * arrays may be host or device memory), remaps its nodes (chunk->nodes: device memory) into merged->nodes and validates
 * them in the same pass; then reads the report back (one stream synchronisation per chunk).  A chunk that fails a check
 * still returns HGS_OK: the caller reads `report`.  tmp: HGS_HIER_MERGE_TMP_BYTES of device memory.
 * hgs_hier_merge_root: node 0's row (after every chunk is placed): the w = alpha * s0 * s1 * s2 weighted moment match
 * of rows 1..k in double, axis-aligned covariance, rotation (1,0,0,0), alpha clipped to [0,1], box = union of the chunk
 * roots' boxes.  Asynchronous on `stream`.
 * Both check sizes and offsets before any HIP call: chunk 1 <= N <= G, merged N in [1 + k, 2^31 - 1] with merged G == N,
 * the chunk's M == the merged M in [1, 64], 0 <= index < k, base_c in [1 + k, merged N - N_c + 1]. */
#define HGS_HIER_MERGE_TMP_BYTES 256
typedef struct hgs_hier_view {
  int64_t G;          /* Gaussian rows */
  int64_t N;          /* nodes */
  int32_t M;          /* SH coefficients per row */
  int32_t reserved;
  float* xyz;         /* [G,3] */
  float* shs;         /* [G,M,3] */
  float* alpha;       /* [G] */
  float* log_scales;  /* [G,3] */
  float* rots;        /* [G,4] */
  int32_t* nodes;     /* [N,7] */
  float* boxes;       /* [N,2,4] */
} hgs_hier_view;
typedef struct hgs_hier_merge_report {
  int32_t first_bad[3]; /* first offending chunk node per check, -1 if none: [0] start != i or count_leafs +
                         * count_merged != 1; [1] a children range outside [1, N) or a negative children count;
                         * [2] node 0's parent != -1, or another node's parent outside [0, N) or not claiming it
                         * (i outside the parent's children range) */
  int32_t reserved;
  int64_t children_sum; /* sum of count_children over the chunk: N - 1 for a valid chunk */
} hgs_hier_merge_report;
int hgs_hier_merge_place(const hgs_hier_view* chunk, int32_t index, int32_t k, int64_t base, const hgs_hier_view* merged,
                         void* tmp, hgs_hier_merge_report* report, hgs_stream_t stream, int device);
int hgs_hier_merge_root(const hgs_hier_view* merged, int32_t k, hgs_stream_t stream, int device);

/* ---------------------------------------------------------------------------
 * Rotation alignment of a hierarchy, in place on the device: the rule of hgs.hierarchy.align_hierarchy (DESIGN.md
 * section 7 f-13).  Opt-in: no other call aligns.  A node's (rotation, scales) pair has 24 equivalent parametrisations:
 * the group G of proper signed permutation matrices M, enumerated as "for perm in permutations(0,1,2): for signs in
 * (1,-1)^3: M[perm[k], k] = signs[k], kept if det M > 0" (element 0 = identity), each with the quaternion g of M and
 * the scale permutation perm (new axis k = +- old axis perm[k]).  Nodes are processed parents before children; the
 * node of depth 0 is untouched.  For node i with parent p whose FINAL quaternion is q'_p: c_j = q_i (x) g_j (Hamilton
 * product, (w,x,y,z)), d_j = <c_j, q'_p>, both in double; j = the first index that maximises |d_j|;
 * q'_i = sign(d_j) c_j with sign(0) = +, rounded to float32 (j = 0: the input's bits or their exact negation);
 * log_scales'_i[k] = log_scales_i[perm_j[k]].  The Gaussian of a node, the norm of its quaternion, xyz, shs, alpha,
 * nodes, boxes and rows at index >= N are unchanged; afterwards |<q'_i, q'_p>| / (|q'_i| |q'_p|) >= (2 + sqrt 2) / 4.
 * nodes int32 [N,7] (only depth and parent are read: any numbering), log_scales [>= N,3], rots [>= N,4] 16-byte aligned,
 * all device memory; 1 <= N <= 2^31 - 1.  tmp: hgs_hier_align_tmp_bytes(N) of device memory, 256-byte aligned.
 * hgs_hier_align_tmp_bytes: host only (no GPU needed); 0 for an N outside [1, 2^31 - 1].
 * hgs_hier_align: sizes and pointers are checked before any HIP call.  The level lists come from the depth column (a
 * stable 8-bit sort of the node ids and a 256-bin count), then one launch per depth; ONE host wait, for the level sizes
 * and the checks.  The hierarchy is validated before anything is written: a failed check returns HGS_ERR_INVALID with
 * the check and its first offending node in the message and in `report`, and leaves log_scales and rots untouched. */
typedef struct hgs_hier_align_report {
  int32_t first_bad[4]; /* first offending node per check, -1 if none: [0] depth outside [0, 255]; [1] a node of depth
                         * > 0 whose parent is outside [0, N); [2] a node of depth > 0 whose parent's depth is not its
                         * own - 1; [3] the second node of depth 0 */
  int32_t roots;        /* nodes of depth 0: 1 for a valid hierarchy */
  int32_t levels;       /* depths in use, counted from 0 up to the first empty one */
  int32_t reserved[2];
} hgs_hier_align_report;
size_t hgs_hier_align_tmp_bytes(int64_t N);
int hgs_hier_align(const int32_t* nodes, int64_t N, float* log_scales, float* rots, void* tmp,
                   hgs_hier_align_report* report, hgs_stream_t stream, int device);

/* ---------------------------------------------------------------------------
 * Trimming a hierarchy on the device: the rule of hgs.hierarchy.trim_hierarchy (DESIGN.md section 4 and section 7
 * f-17).  Input: a hierarchy in this project's layout (one row per node, start == node index, count_leafs +
 * count_merged == 1, contiguous children, every node claimed by its parent), G >= N; rows at index >= N are not read.
 * test(p) = boxes[p,0,3] >= min_extent and, with use_roi != 0, box(p) meets the closed box [roi_lo, roi_hi]: on every
 * axis a, boxes[p,0,a] <= roi_hi[a] and boxes[p,1,a] >= roi_lo[a] (float32 comparisons only: nothing rounds).  Node 0
 * is kept; node n > 0 is kept iff test(parent(n)), so siblings stay or go together.  The N' kept nodes are written in
 * ascending old order: rows (xyz, shs, alpha, log_scales, rots) and boxes copied bit for bit; node records rewritten:
 * depth kept, parent = new_of_old[parent] (-1 at node 0), start = the new index; a node with children whose own test
 * holds keeps its counts and gets start_children = new_of_old[start_children]; a node with children whose own test
 * fails becomes a STUB with a leaf's record (count_leafs 1, count_merged 0, start_children 0, count_children 0); a node
 * without children keeps its record.  old_of_new int32 [N'], new_of_old int32 [N] (-1 at dropped nodes).
 * hgs_hier_trim_tmp_bytes: host only (no GPU needed); 0 for an N outside [1, 2^31 - 1].
 * hgs_hier_trim_plan: one pass over the nodes and a scan; ONE host wait, which reads `report` back.  Four checks, each
 * with its first offending node: the three of hgs_hier_merge_report, and [3] closure -- a kept node n > 0 whose parent
 * p != 0 is dropped (test(parent(p)) fails: the boxes do not nest, or the extents grow downwards).  A failed check
 * returns HGS_ERR_INVALID with the check and the node in the message and in `report`; no output exists yet, so none is
 * touched.  tmp: hgs_hier_trim_tmp_bytes(N) of device memory, 256-byte aligned; it carries the plan to the apply call.
 * hgs_hier_trim_apply: asynchronous on `stream` (the stream of the plan call, or one ordered behind it).  in: the view
 * and tmp of a plan call that returned HGS_OK; out: N = report.kept, G >= N (rows behind N' are not written), the same
 * M, memory that does not overlap the input's.
 * Both check sizes, pointers and alignment before any HIP call: 1 <= N <= 2^31 - 1, N <= G, M in [1, 64]; every array
 * 4-byte aligned, rots and boxes 16-byte aligned (shs is copied in 16-byte pieces where 12 M is a multiple of 16 and
 * both shs bases are 16-byte aligned, in 4-byte pieces otherwise); a min_extent or region bound that is NaN is refused;
 * apply refuses a (device, tmp) pair without a successful plan, an in->N other than the plan's and an out->N other than
 * its kept count. */
typedef struct hgs_hier_trim_args {
  float min_extent;   /* the detail floor (0: none; +inf: the root alone) */
  int32_t use_roi;    /* != 0: also test the node's box against [roi_lo, roi_hi] */
  float roi_lo[3];
  float roi_hi[3];
} hgs_hier_trim_args;
typedef struct hgs_hier_trim_report {
  int32_t first_bad[4]; /* first offending node per check, -1 if none: [0] start != i or count_leafs + count_merged
                         * != 1; [1] a children range outside [1, N) or a negative children count; [2] node 0's parent
                         * != -1, or another node's parent outside [0, N) or not claiming it; [3] a kept node under a
                         * dropped parent */
  int64_t kept;         /* N': nodes of the trimmed hierarchy */
  int64_t stubs;        /* kept nodes with children whose own test fails */
} hgs_hier_trim_report;
size_t hgs_hier_trim_tmp_bytes(int64_t N);
int hgs_hier_trim_plan(const hgs_hier_view* in, const hgs_hier_trim_args* args, void* tmp, hgs_hier_trim_report* report,
                       hgs_stream_t stream, int device);
int hgs_hier_trim_apply(const hgs_hier_view* in, const hgs_hier_view* out, const void* tmp, int32_t* old_of_new,
                        int32_t* new_of_old, hgs_stream_t stream, int device);

/* ---------------------------------------------------------------------------
 * Trimming a hierarchy to the detail a set of views can reach: the rule of hgs.hierarchy.trim_to_views (DESIGN.md
 * section 4 and section 7 f-20), in two additions to the calls above.
 * hgs_hier_reach: regions is a device array float32 [C,6], C closed boxes (lo.xyz, hi.xyz) of camera positions, a
 * single position being lo == hi; finite, lo <= hi (the caller's business: the call does not look).  For every node p,
 * leaves included, in float32 with contraction off and in this order:
 *   d_a(p,c) = fmax(fmax(boxes[p,0,a] - hi_c[a], lo_c[a] - boxes[p,1,a]), 0)       a = x, y, z
 *   d2(p,c)  = (dx*dx + dy*dy) + dz*dz                  D2(p) = min over c of d2(p,c)
 *   reach[p] = D2 > 0 ? boxes[p,0,3] / sqrt(D2) : FLT_MAX
 * -- node_size of the cut with the viewpoint widened to a box: no viewpoint inside any region sees the node larger.  A
 * NaN box coordinate behaves as under fmaxf: d2 is never NaN.  reach: float32 [N] on the device.  Few nodes under many
 * regions are split over the region range and folded with an integer minimum on d2's bit pattern: the result does not
 * depend on the split or on any order.  Asynchronous on `stream`: no host wait.  tmp: hgs_hier_reach_tmp_bytes(N, C) of
 * device memory, 256-byte aligned.  Checked before any HIP call: 1 <= N <= 2^31 - 1, 1 <= C <= 2^24, no null pointer,
 * boxes 16-byte aligned, regions and reach 4-byte aligned.
 * hgs_hier_reach_tmp_bytes: host only (no GPU needed); 0 for an N or a C out of range.
 * hgs_hier_trim_plan_keyed: hgs_hier_trim_plan with one more conjunct in test: key[p] >= key_floor, key a device
 * float32 [N] (4-byte aligned).  With key = reach and key_floor = a granularity tau, node n > 0 is kept iff some view of
 * the set can see its parent at a size >= tau (and the parent passes the floor and the region of `args`).  A NaN key
 * never passes; a NaN key_floor is refused.  Same checks (closure fails where the boxes do not nest:
 * hgs.refit_hierarchy mends that), same single host wait, same report, same tmp (hgs_hier_trim_tmp_bytes(N)) and the
 * same plan record: hgs_hier_trim_apply follows it unchanged.  key is not read by apply. */
size_t hgs_hier_reach_tmp_bytes(int64_t N, int64_t C);
int hgs_hier_reach(const float* boxes, int64_t N, const float* regions, int64_t C, float* reach, void* tmp,
                   hgs_stream_t stream, int device);
int hgs_hier_trim_plan_keyed(const hgs_hier_view* in, const hgs_hier_trim_args* args, const float* key, float key_floor,
                             void* tmp, hgs_hier_trim_report* report, hgs_stream_t stream, int device);

/* ---------------------------------------------------------------------------
 * Similarity transform of a hierarchy on the device: the rule of hgs.hierarchy.transform_hierarchy (DESIGN.md section 4
 * and section 7 f-18).  The map is x' = s R x + t, R a proper rotation, s > 0.  All G rows are transformed (a skybox
 * tail behind the N nodes included), the N boxes are transformed, nodes and alpha are copied bit for bit.  Every product
 * and sum in double, every sum left to right, no contraction, one rounding to float32:
 *   xyz'_a        = ((R[3a] x_0 + R[3a+1] x_1) + R[3a+2] x_2) s + t_a
 *   rots'         = q (x) rots, the Hamilton product (w,x,y,z); norms are not renormalised
 *   log_scales'_k = log_scales_k + log_s
 *   shs           band 0 (coefficient 0) keeps its bits; band l = 1, 2, 3 (coefficients l^2 .. l^2 + 2 l), per channel:
 *                 c'_m = sum_m' D_l[m (2 l + 1) + m'] c_m', M = 1, 4, 9 or 16 only (whole bands)
 *   boxes         lo'_a = (sum_b (R_ab >= 0 ? R_ab lo_b : R_ab hi_b)) s + t_a, hi'_a the same with lo and hi swapped;
 *                 boxes'[n,0,3] = max_a (hi'_a - lo'_a) in float32 on the rounded values; boxes[n,1,3] is copied
 * The device does not derive the SH blocks: it consumes D1, D2, D3 as given (hgs.hierarchy.sh_rotation_blocks), so the
 * spec and the kernel share every bit of them.  Each array of `out` is the same pointer as in `in` (in place) or memory
 * that does not overlap any array of `in`; both views have the same G, N and M.  Asynchronous on `stream`, no host wait.
 * Checked before any HIP call (HGS_ERR_INVALID, hgs_last_error names it, nothing is written): 1 <= N <= G <= 2^31 - 1;
 * an output array that overlaps its input array without being that array is refused; every array 4-byte aligned, rots and boxes 16-byte aligned (shs moves in 16-byte pieces where 12 M is a multiple of 16
 * and both shs bases are 16-byte aligned, in 4-byte pieces otherwise); M in {1, 4, 9, 16}; |R R^T - I| <= 1e-9 and
 * det R > 0; q reproduces R to 1e-9; s and t finite, s > 0; |log_s - log(s)| <= 1e-12; every D_l orthogonal to 1e-9 and
 * consistent with R: D_l^T b_l(d) = b_l(R^T d) to 1e-9 at 16 fixed directions, b_l the renderer's basis of band l. */
typedef struct hgs_hier_transform_args {
  double R[9];    /* row-major */
  double q[4];    /* the quaternion of R, (w,x,y,z) */
  double s;
  double log_s;   /* log(s) */
  double t[3];
  double D1[9];   /* SH blocks, row-major: c' = D_l c */
  double D2[25];
  double D3[49];
} hgs_hier_transform_args;
int hgs_hier_transform(const hgs_hier_view* in, const hgs_hier_view* out, const hgs_hier_transform_args* args,
                       hgs_stream_t stream, int device);

/* ---------------------------------------------------------------------------
 * Refitting a hierarchy's boxes on the device, bottom-up: the rule of hgs.hierarchy.refit_boxes (DESIGN.md section 4
 * and section 7 f-19).  Only boxes change: the rows, the node records and rows at index >= N are not written (rows at
 * index >= N are not read).  Input: a hierarchy in this project's layout, G >= N.
 *   a leaf (count_children == 0), by leaf_mode, with x its xyz and s_k = exp(double(log_scales_k)):
 *     0 keep       the input box, all eight floats, bit for bit
 *     1 cube       e = 3 max_k s_k; lo_a = f32(x_a - e), hi_a = f32(x_a + e) (the builder's leaf rule on the stored rows)
 *     2 ellipsoid  q^ = q / |q| with |q| = sqrt(((w w + x x) + y y) + z z), R the rotation matrix of q^,
 *                  h_a = 3 sqrt(((R_a0 R_a0) s_0^2 + (R_a1 R_a1) s_1^2) + (R_a2 R_a2) s_2^2); lo_a = f32(x_a - h_a),
 *                  hi_a = f32(x_a + h_a): the AABB of the 3 sigma ellipsoid
 *     in double, every sum left to right, no contraction, one rounding to float32
 *   a node with children: lo = min, hi = max over the FINAL boxes of its children [start_children, start_children +
 *     count_children), children before parents; its own Gaussian is not included (the builder's and the merger's rule);
 *     min and max are exact
 *   every written box: boxes[n,0,3] = max_a (hi_a - lo_a), a float32 subtraction on the rounded values; boxes[n,1,3] is
 *     copied from the input (a kept leaf keeps its boxes[n,0,3] too)
 * The output nests exactly: rounding is monotone, and a parent's extent is >= its child's.
 * boxes_out float [N,2,4]: in->boxes itself (in place) or device memory that does not overlap it.  tmp:
 * hgs_hier_refit_tmp_bytes(N) of device memory, 256-byte aligned.
 * hgs_hier_refit_tmp_bytes: host only (no GPU needed); 0 for an N outside [1, 2^31 - 1].
 * hgs_hier_refit: checked before any HIP call (HGS_ERR_INVALID, hgs_last_error names it): 1 <= N <= 2^31 - 1, N <= G,
 * M in [1, 64]; every array 4-byte aligned, rots, boxes and boxes_out 16-byte aligned; a boxes_out that overlaps
 * in->boxes without being that array; a leaf_mode outside {0, 1, 2}.  Then one pass over the nodes validates the
 * hierarchy and evaluates every leaf's box for its test, a stable 8-bit sort of the node ids by depth gives the level
 * lists, and ONE host wait reads `report` back.  A failed check returns HGS_ERR_INVALID with the check and its first
 * offending node in the message and in `report`; nothing has been written to boxes_out then.  After it: a pass over
 * the leaves and one launch per depth from the deepest level with children up to 0, asynchronous on `stream`. */
typedef struct hgs_hier_refit_report {
  int32_t first_bad[7]; /* first offending node per check, -1 if none: [0] start != i or count_leafs + count_merged
                         * != 1; [1] a children range outside [1, N) or a negative children count; [2] node 0's parent
                         * != -1, or another node's parent outside [0, N) or not claiming it; [3] depth outside [0, 255];
                         * [4] a depth that is not the parent's + 1 (without a parent in [0, N): a depth != 0); [5] the
                         * second node of depth 0; [6] a leaf whose box is not finite or has lo > hi on an axis (NaN or
                         * inf rows, a zero quaternion under ellipsoid, a bad kept box under keep) */
  int32_t levels;       /* depths in use, counted from 0 up to the first empty one */
  int64_t leaves;       /* nodes with count_children == 0 */
  int64_t children_sum; /* sum of count_children over the valid children ranges: N - 1, or the call is refused (two
                         * nodes claim the same children) */
} hgs_hier_refit_report;
size_t hgs_hier_refit_tmp_bytes(int64_t N);
int hgs_hier_refit(const hgs_hier_view* in, float* boxes_out, int32_t leaf_mode, void* tmp, hgs_hier_refit_report* report,
                   hgs_stream_t stream, int device);

/* ---------------------------------------------------------------------------
 * Removing leaves from a hierarchy on the device and re-merging their ancestors: the rule of
 * hgs.hierarchy.prune_hierarchy (this project's own rule).  Input: a hierarchy
 * in this project's layout, G >= N; rows at index >= N are not read.
 *   removed  a node with count_children == 0 is removed iff a criterion of `args` holds, all in float32:
 *            its mean lies inside one of the remove_boxes closed boxes (a NaN coordinate is never inside); use_keep_box
 *            and its mean is not inside [keep_lo, keep_hi]; use_min_opacity and not (alpha >= min_opacity);
 *            use_max_scale and not (max_k log_scales_k <= log_max_scale) -- the caller passes the LOGARITHM, rounded to
 *            float32 once; `remove` (NULL, or a device uint8 [N]) is nonzero at the node.  Entries of `remove` at nodes
 *            with children are ignored.
 *   alive    bottom-up: a leaf iff it is not removed, a node with children iff one of its children is.  Dead nodes are
 *            dropped; a dead node 0 refuses the call ("every leaf would be removed").
 *   dirty    an alive node with children one of whose children is dead or dirty.
 *   records  the N' alive nodes in ascending old order (surviving children stay contiguous): depth, count_leafs and
 *            count_merged kept; parent = new_of_old[parent] (-1 at node 0), start = the new index, start_children =
 *            new_of_old[first surviving child], count_children = the surviving children (1 is allowed: such chains are
 *            not spliced); a node without children keeps its record but parent and start.
 *   rows     leaves and clean nodes: rows and boxes bit for bit.  A dirty node: its box is the union of its surviving
 *            children's FINAL boxes, boxes[n,0,3] the largest edge (a float32 subtraction), boxes[n,1,3] copied -- in
 *            every re-merge mode; its row, deepest level first, from its surviving children's final float32 rows:
 *            w_c = the weight the builder carries: alpha_c exp(ls_c0) exp(ls_c1) exp(ls_c2) of a child without
 *            children, max(sum of its surviving children's weights, 1e-30) of a child with children (the sum over its
 *            surviving leaves, not the product of its own merged row); f_c = w_c / max(sum_c w_c, 1e-30); mean = sum f_c x_c;
 *            covariance = sum f_c (R_c diag(s_c^2) R_c^T + d_c d_c^T), d_c = x_c - mean, R_c the matrix of the stored
 *            quaternion (w,x,y,z); SH and opacity = the f-weighted averages, opacity clipped to [0, 1]; scales and
 *            rotation = the builder's cyclic Jacobi solve and parametrisation (eigenvalues ascending, clamped at 1e-12,
 *            each axis' largest component positive, column 0 negated if improper).  All in double, one rounding.
 *   remerge  HGS_HIER_PRUNE_REMERGE_DIRTY: as above; _NONE: dirty nodes keep their rows (boxes are still unions): a
 *            topology-only prune; _ALL: every alive node with children gets its row again (clean ones keep their boxes).
 * hgs_hier_prune_tmp_bytes: host only (no GPU needed); 0 for an N outside [1, 2^31 - 1].
 * hgs_hier_prune_plan: the checks of hgs_hier_refit_report [0..5] and the count_children sum, the level lists, the
 * removal test, alive and dirty bottom-up (one launch per depth), a scan; TWO host waits; the second reads `report`.  A
 * failed check or a dead root returns HGS_ERR_INVALID with the check and the node in the message and in `report`; no
 * output exists yet, so none is touched.  tmp: hgs_hier_prune_tmp_bytes(N) of device memory, 256-byte aligned; it
 * carries the plan to the apply call.
 * hgs_hier_prune_apply: asynchronous on `stream` (the plan's, or one ordered behind it).  out: N = report.kept, G >= N,
 * the same M, memory that does not overlap the input's.  old_of_new int32 [N'], new_of_old int32 [N] (-1 at the dead).
 * Both check sizes, pointers and alignment before any HIP call (as hgs_hier_trim_plan / _apply do); more than 16 remove
 * boxes, a NaN bound or threshold and a remerge outside {0, 1, 2} are refused; apply refuses a (device, tmp) pair without
 * a successful plan, an in->N other than the plan's, an out->N other than its kept count, and an output array that
 * overlaps its input array. */
#define HGS_HIER_PRUNE_MAX_BOXES 16
#define HGS_HIER_PRUNE_REMERGE_NONE 0
#define HGS_HIER_PRUNE_REMERGE_DIRTY 1
#define HGS_HIER_PRUNE_REMERGE_ALL 2
typedef struct hgs_hier_prune_args {
  int32_t remove_boxes;     /* how many of remove_lo / remove_hi are in use: 0 .. 16 */
  int32_t use_keep_box;
  int32_t use_min_opacity;
  int32_t use_max_scale;
  float remove_lo[HGS_HIER_PRUNE_MAX_BOXES][3];
  float remove_hi[HGS_HIER_PRUNE_MAX_BOXES][3];
  float keep_lo[3];
  float keep_hi[3];
  float min_opacity;
  float log_max_scale;      /* float32(log(S)) */
} hgs_hier_prune_args;
typedef struct hgs_hier_prune_report {
  int32_t first_bad[6];   /* first offending node per check, -1 if none: hgs_hier_refit_report's [0] .. [5] */
  int32_t levels;         /* depths in use */
  int32_t root_dead;      /* != 0: every leaf would be removed (the call is refused) */
  int64_t kept;           /* N': alive nodes */
  int64_t removed_leaves; /* leaves a criterion removes */
  int64_t dead;           /* N - N' */
  int64_t dirty;          /* alive nodes with a dead or dirty child */
  int64_t single_child;   /* alive nodes left with exactly one child */
  int64_t children_sum;   /* N - 1, or the call is refused */
} hgs_hier_prune_report;
size_t hgs_hier_prune_tmp_bytes(int64_t N);
int hgs_hier_prune_plan(const hgs_hier_view* in, const hgs_hier_prune_args* args, const uint8_t* remove, void* tmp,
                        hgs_hier_prune_report* report, hgs_stream_t stream, int device);
int hgs_hier_prune_apply(const hgs_hier_view* in, const hgs_hier_view* out, const void* tmp, int32_t remerge,
                         int32_t* old_of_new, int32_t* new_of_old, hgs_stream_t stream, int device);

/* ---------------------------------------------------------------------------
 * Fused SSIM loss (hgs.loss.ssim): the standard SSIM of the reference's loss -- an 11-tap
 * Gaussian window (sigma 1.5, normalised to sum 1) applied separably, zero padding, C1 = 0.01^2, C2 = 0.03^2 -- of
 * img1 against img2, both float32 [N,C,H,W] contiguous on the device, and its gradient with respect to img1.
 * hgs_ssim_tmp_bytes: host only (no GPU needed); 0 for bad sizes (the reason in hgs_last_error).
 * hgs_ssim_fwd: out_image [N] = mean SSIM per image, out_mean [1] = mean over every channel and pixel.  maps:
 * NULL, or [3,N,C,H,W] floats that receive the per-pixel partials the backward needs.  tmp: hgs_ssim_tmp_bytes,
 * 8-byte aligned.  The sums are added in a fixed order (no atomics): two calls give bit-identical results.
 * hgs_ssim_bwd: grad_img1 [N,C,H,W] from the forward's maps; grad_out is the upstream gradient on the device, one
 * value (per_image = 0: of out_mean) or N values (per_image = 1: of out_image).
 * All three check sizes before any HIP call: N, C, H, W >= 1, N*C*H*W (x 12 bytes of maps) within int64, at most
 * 16 777 215 tiles of 32x16 pixels over all N*C planes (one 256-thread workgroup per tile in a 1-D grid, whose size in
 * work-items is a 32-bit count).  Forward and backward are asynchronous on `stream` (no host synchronisation). */
size_t hgs_ssim_tmp_bytes(int32_t N, int32_t C, int32_t H, int32_t W);
int hgs_ssim_fwd(const float* img1, const float* img2, int32_t N, int32_t C, int32_t H, int32_t W, float* out_image,
                 float* out_mean, float* maps, void* tmp, hgs_stream_t stream, int device);
int hgs_ssim_bwd(const float* img1, const float* img2, const float* maps, const float* grad_out, int32_t per_image,
                 int32_t N, int32_t C, int32_t H, int32_t W, float* grad_img1, hgs_stream_t stream, int device);

/* ---------------------------------------------------------------------------
 * Fused training loss (hgs.loss.photometric_loss): the whole loss of the reference's three
 * training scripts and its gradients.  Per pixel and output channel j, in the reference's order of operations:
 *   u_j = sum_i r_i E[i][j] + E[j][3]   (gaussian_renderer/__init__.py:115-117; u = r when exposure is NULL)
 *   v_j = min(max(u_j, 0), 1)           (gaussian_renderer/__init__.py:118; only with clamp != 0; the gradient passes
 *                                        where 0 <= u_j <= 1, both ends included)
 *   x_j = v_j m                         (train_single.py:102-104, train_post.py:134-137; m = 1 when alpha_mask is NULL)
 *   L1 = mean |x - gt| (d|t|/dt = sign t, sign 0 = 0), S = SSIM(x, gt) as hgs_ssim_fwd, D = mean |(d - d_mono) m_d|
 *   loss = (1 - lambda_dssim) L1 + lambda_dssim (1 - S) + depth_weight D
 *                                       (train_single.py:106-117, train_post.py:139-140, train_coarse.py:99-105)
 * All means run over every element of the batch.  Every tensor is float32, contiguous, on the device.
 * hgs_photo_tmp_bytes: host only (no GPU needed); 0 for bad sizes (the reason in hgs_last_error).
 * hgs_photo_fwd: out [4] = loss, L1, S, D (D = 0 without a depth term).  maps: NULL, or [3,N,C,H,W] floats that receive
 *   the per-pixel SSIM partials the backward needs.  tmp: hgs_photo_tmp_bytes, 8-byte aligned.  Two launches (the tiles,
 *   then a fixed-order reduction of the per-workgroup partials, which are kept in double).
 * hgs_photo_bwd: from the forward's maps and the upstream gradient of `loss` on the device (grad_out [1]):
 *   grad_rendered [N,C,H,W]; grad_exposure [N,3,4] or NULL (12 sums per image over all pixels, accumulated in double and
 *   reduced in a fixed order); grad_invdepth [N,H,W] or NULL = depth_weight grad_out / (N H W) sign((d - d_mono) m_d)
 *   m_d.  tmp as for the forward.  One launch, plus the reduction when grad_exposure is given.
 * No atomics: two calls give bit-identical results.  All three check, before any HIP call: the sizes as hgs_ssim_*
 * does (the tiling is the same), C == 3 with an exposure, the depth triple given whole or not at all, lambda_dssim in
 * [0, 1], a finite depth_weight, grad_exposure / grad_invdepth only with exposure / invdepth.  Asynchronous on
 * `stream` (no host synchronisation). */
typedef struct hgs_photo_args {
  const float* rendered;       /* [N,C,H,W] r */
  const float* gt;             /* [N,C,H,W] */
  const float* exposure;       /* [N,3,4] row-major, or NULL */
  const float* alpha_mask;     /* [N,H,W], or NULL */
  const float* invdepth;       /* [N,H,W] d, or NULL (then the next two are NULL too) */
  const float* mono_invdepth;  /* [N,H,W] */
  const float* depth_mask;     /* [N,H,W] */
  int32_t N, C, H, W;
  int32_t clamp;               /* 0 / 1 */
  int32_t reserved;
  double lambda_dssim;
  double depth_weight;
} hgs_photo_args;
size_t hgs_photo_tmp_bytes(int32_t N, int32_t C, int32_t H, int32_t W);
int hgs_photo_fwd(const hgs_photo_args* args, float* out, float* maps, void* tmp, hgs_stream_t stream, int device);
int hgs_photo_bwd(const hgs_photo_args* args, const float* maps, const float* grad_out, float* grad_rendered,
                  float* grad_exposure, float* grad_invdepth, void* tmp, hgs_stream_t stream, int device);

/* ---------------------------------------------------------------------------
 * Adaptive density control as one stream compaction (hgs.densify): replaces the torch chain of
 * the reference's GaussianModel.densify_and_prune (scene/gaussian_model.py:528-685, called from
 * train_single.py:150-151).  Per row r of P, with F protected leading rows (scaffold_points) and d = percent_dense *
 * extent:  g = accum (NaN -> 0), o = sigmoid(opacity), m = max_k exp(scaling_k), w = max_radii2D * o^(1/5);
 *   clone = |g| w >= max_grad and o > 0.15 and m <= d and r >= F;   split = g w >= max_grad and o > 0.15 and m > d and
 *   r >= F (no absolute value, gaussian_model.py:625);   low = o < min_opacity.
 * Output rows, each block in ascending r: originals with not split and not (low and r >= F); one copy of every clone
 * row with not low; child 0 of every split row with not low; child 1 of the same rows.  The k-th split row (ascending
 * r, pruned ones included) owns the noise rows z[k] and z[S + k] of noise [2S,3];  child j: xyz' = xyz + R(q / |q|)
 * (exp(scaling) * z_j) with R of utils/general_utils.py:82-103, scaling' = log(exp(scaling) / 1.6), the rest copied;
 * moments of new rows are zero.
 * hgs_densify_tmp_bytes: host only (no GPU needed); 0 for a P outside [0, 2^31 - 1] (the reason in hgs_last_error).
 * hgs_densify_plan: accum [P], radii [P], opacity [P], scaling [P,3] (device, raw as the optimizer holds them); tmp:
 *   hgs_densify_tmp_bytes(P) bytes of device memory, 256-byte aligned; totals: four int64 that the device can write
 *   (device memory, or pinned device-mapped memory from hgs_host_alloc): kept originals, kept clones, split rows S,
 *   kept split rows.  wait != 0: the call returns after the stream has drained (polled; HGS_BLOCKING_WAIT honoured), so
 *   that host-mapped totals can be read; otherwise it is asynchronous on `stream`.
 * hgs_densify_apply: up to HGS_ADAM_MAX_TENSORS tensors of P rows with the plan left in tmp; totals: the plan's four
 *   values ON THE HOST; every tensor's dst (and moments, if it has any: both or neither) holds totals[0] + totals[1] +
 *   2 totals[3] rows.  kind: HGS_DENSIFY_XYZ / HGS_DENSIFY_SCALING get the child arithmetic (row_len 3), everything
 *   else is copied.  scaling [P,3], rotation [P,4] and noise [2S,3] are read for the children of an XYZ tensor.
 *   Asynchronous on `stream`.  No atomics: two calls give bit-identical results.
 * All check sizes, null pointers, 0 <= F <= P, max_grad > 0 and rows x row_len overflow before any HIP call; no state is
 * kept between calls. */
#define HGS_DENSIFY_COPY 0
#define HGS_DENSIFY_XYZ 1
#define HGS_DENSIFY_SCALING 2
typedef struct hgs_densify_tensor {
  const float* src;          /* [P, row_len] */
  const float* exp_avg;      /* [P, row_len] or NULL (then exp_avg_sq is NULL too and no moments are written) */
  const float* exp_avg_sq;
  float* dst;                /* [P', row_len] */
  float* dst_exp_avg;
  float* dst_exp_avg_sq;
  int32_t row_len;
  int32_t kind;              /* HGS_DENSIFY_* */
} hgs_densify_tensor;
size_t hgs_densify_tmp_bytes(int64_t P);
int hgs_densify_plan(const float* accum, const float* radii, const float* opacity, const float* scaling, int64_t P,
                     int64_t F, float max_grad, float min_opacity, float d, void* tmp, int64_t* totals, int32_t wait,
                     hgs_stream_t stream, int device);
int hgs_densify_apply(const hgs_densify_tensor* tensors, int32_t n_tensors, int64_t P, const int64_t* totals,
                      const float* scaling, const float* rotation, const float* noise, const void* tmp,
                      hgs_stream_t stream, int device);

/* ---------------------------------------------------------------------------
 * The bookkeeping between loss.backward() and the next render as two launches (hgs.step):
 * replaces the ~twenty torch launches and four device-to-host waits of train_single.py:144-186, train_post.py:164-192
 * and train_coarse.py:110-145.  P model rows, six (or any <= HGS_ADAM_MAX_TENSORS per call) parameter tensors [P, row_len]
 * float32 with gradient and Adam moments.  Three parts, each optional, in this order:
 *  1. Statistics (train_single.py:147-148, train_coarse.py:110; scene/gaussian_model.py:687-689).  Either (a) raw radii
 *     [n] int32 as the rasterizer returns them, rendered row i being model row r = indices[i] (or r = i without
 *     indices, n <= P) and visible iff radii[i] > 0; or (b) visible [n] int64 model rows with their compacted radii [n],
 *     the pair render() returns, every listed row visible.  For every visible row r:
 *       max_radii2D[r] = max(max_radii2D[r], float(radius));
 *       if accum: accum[r] = max(sqrt(g[r,0]^2 + g[r,1]^2), accum[r]) with g = means2D_grad [P,3];  denom[r] += 1.
 *     max is torch.maximum's: a NaN operand gives NaN.  A row may be listed at most once (not checked; the reference's
 *     indexed assignment is undefined there too); a row outside [0, P) is skipped.
 *  2. Optimizer step (train_single.py:162-178, train_post.py:167-192).  Row r is LOCKED if r < lock_head or r >= P -
 *     lock_tail or lock_mask[r] != 0.  The effective gradient of a tensor flagged HGS_STEP_LOCKABLE is 0 at a locked row,
 *     the gradient everywhere else.  select_all == 0: the selected rows are those whose effective opacity gradient
 *     (opacity_grad [P]; lock_opacity: opacity is lockable) is != 0 -- and if no row is selected, every row is
 *     (train_single.py:173-177 with scene/OurAdam.py:214: an empty `relevant` takes the dense path).  select_all != 0:
 *     every row (train_post.py:191).  Selected rows of every tensor take exactly hgs_adam_step's update with the
 *     effective gradient; unselected rows are not read (but for the scaling rows part 3 looks at).  A tensor with
 *     grad == NULL is not updated (a densification iteration left no gradients).
 *  3. Size clamp (train_single.py:180-186, train_coarse.py:141-145), on the tensor flagged HGS_STEP_SCALING (row_len 3),
 *     on its value after part 2, for every row r >= protect_head: if max_k exp(s[r,k]) > clamp_threshold then
 *     s[r,k] = log(exp(s[r,k]) * 0.8) for all k.  Moments are not touched.  A row whose maximum is within a relative
 *     1e-5 of the threshold may go either way (f-8's knife-edge band).
 * Not reproduced, on purpose: the [k,2] `relevant` of train_coarse.py:133 (the coarse configuration is expressed as a
 * lock of `scaling` alone with lock_head = skybox_points, clamp (0.1 extent, skybox_points) and selection by opacity
 * gradient); the exposure optimizer (12 floats per camera, stays torch); reset_opacity; the zeroed slices of the .grad
 * tensors themselves (unobservable after zero_grad(set_to_none=True)).
 * hgs_step_tmp_bytes: host only (no GPU needed); 0 for a P outside [0, 2^31 - 1] (the reason in hgs_last_error).
 * hgs_step_select: part 1, and one class byte per model row (selected / locked / clamp candidate) plus one "some row
 *   was selected" word into tmp (hgs_step_tmp_bytes(P) bytes of device memory, 256-byte aligned).  The word is zeroed
 *   on the stream, set by wave ballot and one vector store per wave.  n == 0: no statistics.
 * hgs_step_apply: parts 2 and 3 from the class bytes and the word the select call of the SAME args left in tmp; the
 *   word chooses the dense fallback inside the kernel.  One launch per call.  clamp != 0 needs one HGS_STEP_SCALING
 *   tensor among `tensors`.
 * Both are asynchronous on `stream`: nothing comes back to the host, nothing waits.  Both check sizes (P, n >= 0,
 * row lengths, lock_head + lock_tail <= P, 0 <= protect_head <= P), null combinations and the threshold before any HIP
 * call; P == 0 or nothing to do returns HGS_OK without a launch.  No atomics: two calls give bit-identical results. */
#define HGS_STEP_LOCKABLE 1   /* hgs_step_tensor.flags: in lock_names */
#define HGS_STEP_SCALING 2    /* the tensor the size clamp acts on; handled a row (3 floats) at a time */
typedef struct hgs_step_args {
  int64_t P;
  int64_t n;                  /* rendered rows (a) or listed rows (b); 0: no statistics */
  const int32_t* radii;       /* [n] */
  const int32_t* indices;     /* (a) [n] or NULL */
  const int64_t* visible;     /* (b) [n]; NULL: form (a) */
  const float* means2D_grad;  /* [P,3]; needed with accum */
  float* max_radii2D;         /* [P]; needed with n > 0 */
  float* accum;               /* [P] or NULL (then denom is NULL too) */
  float* denom;               /* [P] */
  const float* opacity_grad;  /* [P]; NULL: no row is marked selected (apply then updates nothing unless select_all) */
  const uint8_t* lock_mask;   /* [P] or NULL */
  int64_t lock_head, lock_tail;
  int64_t protect_head;       /* rows below are never clamped */
  int32_t select_all;
  int32_t lock_opacity;
  int32_t clamp;              /* != 0: part 3 with clamp_threshold (positive, finite) */
  float clamp_threshold;
} hgs_step_args;
typedef struct hgs_step_tensor {
  hgs_adam_tensor adam;       /* as hgs_adam_step takes it; grad == NULL: no update (clamp only) */
  int32_t flags;              /* HGS_STEP_* */
  int32_t reserved;
} hgs_step_tensor;
size_t hgs_step_tmp_bytes(int64_t P);
int hgs_step_select(const hgs_step_args* args, void* tmp, hgs_stream_t stream, int device);
int hgs_step_apply(const hgs_step_args* args, const hgs_step_tensor* tensors, int32_t n_tensors, const void* tmp,
                   hgs_stream_t stream, int device);

/* ---------------------------------------------------------------------------
 * Direct (two-shot) SUM all-reduce over peer pointers: the exchange step of per-view data parallelism (SURVEY.md
 * section 8(e); the reference itself is single-GPU: train_single.py:57-59 renders one camera per step, nothing to
 * replace).  One process per GPU; every rank allocates its gradient bucket and a small flag block with hgs_p2p_alloc,
 * exports both (hipIpc), opens its peers' and then calls hgs_p2p_allreduce_sum: rank r sums shard r of ALL buckets in
 * rank order (reading the peers' memory over xGMI: all links at once, where a ring is bound by one) and writes it back
 * into its own bucket, then copies the other ranks' reduced shards from their buckets -- every rank ends with
 * bit-identical sums.  Three flag barriers per call (release / acquire at system scope, bounded spin: a peer that
 * never arrives sets the error word instead of hanging the device).  world <= HGS_P2P_MAX_WORLD.
 * Opt-in (hgs/dp.py: HGS_DP_ALLREDUCE=direct); the default exchange is RCCL's all-reduce through torch.distributed.
 * ------------------------------------------------------------------------- */
#define HGS_P2P_MAX_WORLD 8
#define HGS_P2P_HANDLE_BYTES 64
#define HGS_P2P_FLAG_BYTES 256   /* size of a rank's flag block: barrier words 0..2, error word 3 */
/* flags: bit 0 = uncached memory (the flag block); bit 1 = fine-grained device memory (a bucket that must be coherent
 * across devices INSIDE a kernel; the protocol below only hands buckets over at kernel boundaries and uses ordinary
 * memory, flags = 0); a barrier that waits longer than HGS_P2P_TIMEOUT_S (default 60) sets the sticky error word and
 * makes the rank's reduce / gather write NaN (csrc/p2p.hip) */
int hgs_p2p_alloc(size_t bytes, int32_t flags, void** ptr, int device);
int hgs_p2p_free(void* ptr, int device);
int hgs_p2p_export(void* ptr, uint8_t handle[HGS_P2P_HANDLE_BYTES], int device);
int hgs_p2p_open(const uint8_t handle[HGS_P2P_HANDLE_BYTES], void** ptr, int device);
int hgs_p2p_close(void* ptr, int device);
/* bufs[world] / flag_blocks[world]: device pointers valid in THIS process (own allocation at [rank], opened peers
 * elsewhere).  Reduces the floats [offset, offset + n) of every bucket; offset and n multiples of 4.  epoch: a counter
 * that every rank increments by one per call (all ranks must make the same sequence of calls).  Stream-ordered: the
 * buckets must have been written by work enqueued earlier on `stream`; the result is complete, and the bucket may be
 * overwritten, after the calls' kernels.  The error word (flag block word 3) is non-zero after a timed-out barrier. */
int hgs_p2p_allreduce_sum(int32_t rank, int32_t world, void* const* bufs, void* const* flag_blocks, size_t offset,
                          size_t n, uint32_t epoch, hgs_stream_t stream, int device);

/* ---------------------------------------------------------------------------
 * Budgeted residency of a hierarchy's attribute rows ("VRAM-budgeted streaming LOD": the `--budget <MB>` of the
 * reference's hierarchy viewer, README.md:233-235 -- "this only defines the budget for the SCENE representation" --
 * whose implementation lives in the un-vendored SIBR viewer; BASELINE configs[4] names it).  Opt-in layer BESIDE the
 * drop-in path (hgs/residency.py): the attributes of ALL rows stay in pinned, device-mapped HOST memory
 * (hgs_host_alloc) as packed rows (HGS_RESID_HOST_ROW_FLOATS); the GPU holds `B` rows in slot arrays.  Per view, after
 * the LOD cut and its weights:
 *   hgs_resid_mark    every row the cut needs (node row of each entry, and its parent row unless `weights` -- nullable,
 *                     the entries' interpolation weights -- says the weight is exactly 1: the in-op LOD gather does
 *                     not read that parent, and po then repeats the node's slot): resident -> stamped with the
 *                     frame number; absent -> appended ONCE to the miss list (slot_of: >= 0 slot, -1 absent, -2 queued
 *                     this frame); ro / po receive the slots of the resident rows.  Waits; *miss_count_host = rows
 *                     queued -- also when the call fails with HGS_ERR_INVALID on an index outside [0, G): the caller
 *                     has to take them out of the queue again (slot_of back to -1).
 *   hgs_resid_evict   when the free list is shorter than the miss list: frees the slots that have gone unused for
 *                     the longest (age histogram on the device, threshold chosen on the host; rows stamped this frame
 *                     are never evicted).  HGS_ERR_CAPACITY if even that is not enough: the working set of the view
 *                     exceeds the budget -- the caller raises tau, as the reference's viewer "auto-regulates".
 *   hgs_resid_fetch   assigns free slots to the missing rows and copies their attributes from the packed host rows
 *                     (HGS_RESID_HOST_ROW_FLOATS) into the slot arrays: ONE kernel reading host memory directly (zero
 *                     copy over PCIe, one coalesced 256-byte read per row), no staging buffer, no host-side gather.
 *   hgs_resid_remap   render_indices / parent_indices (Gaussian rows) -> slot indices, for the in-op LOD path of the
 *                     rasterizer (hgs_raster_args.lod_*) running on the slot arrays.
 * slot_of int32 [G] (initialised to -1), stamp uint32 [B], id_of_slot int32 [B] (initialised to -1), free_list int32
 * [B] (initialised to B-1 .. 0: slot 0 is handed out first), counters uint32 [HGS_RESID_COUNTER_WORDS] (device
 * scratch), miss_ids int32
 * [2 x capacity of the index arrays].  All calls are ordered on `stream`.
 * ------------------------------------------------------------------------- */
#define HGS_RESID_COUNTER_WORDS 68
/* host side of the budgeted residency: one packed row of 64 floats (256 B = four 64-byte PCIe reads) per Gaussian, in
 * memory from hgs_host_alloc:  [0, 3 M) SH coefficients, [48, 52) rotation, [52, 55) mean, [55, 58) scale, [58] opacity */
#define HGS_RESID_HOST_ROW_FLOATS 64
typedef struct hgs_resid_rows {
  float* means3D;    /* [rows, 3]    */
  float* shs;        /* [rows, M, 3] */
  float* opacities;  /* [rows]       */
  float* scales;     /* [rows, 3]    */
  float* rotations;  /* [rows, 4]    */
} hgs_resid_rows;
void* hgs_host_alloc(size_t bytes);      /* pinned host memory mapped into every device's address space; NULL on failure */
void hgs_host_free(void* p);
int hgs_resid_mark(const int32_t* render_indices, const int32_t* parent_indices, const float* weights, int32_t n, int32_t G,
                   int32_t* slot_of, uint32_t* stamp, uint32_t frame, int32_t* miss_ids, uint32_t* counters,
                   int32_t* ro, int32_t* po, uint32_t* miss_count_host, hgs_stream_t stream, int device);
int hgs_resid_evict(uint32_t* stamp, int32_t* id_of_slot, int32_t* slot_of, int32_t B, uint32_t frame, uint32_t need,
                    int32_t* free_list, uint32_t* counters, uint32_t* free_top_inout_host, hgs_stream_t stream,
                    int device);
int hgs_resid_fetch(const int32_t* miss_ids, uint32_t m, const int32_t* free_list, uint32_t free_top, int32_t* slot_of,
                    int32_t* id_of_slot, uint32_t* stamp, uint32_t frame, const float* host_rows_packed,
                    const hgs_resid_rows* slot_rows, int32_t M, hgs_stream_t stream, int device);
int hgs_resid_remap(const int32_t* render_indices, const int32_t* parent_indices, const float* weights, int32_t n,
                    const int32_t* slot_of, int32_t* ro, int32_t* po, hgs_stream_t stream, int device);

/* Half-precision host rows (opt-in): 128 bytes per Gaussian = two 64-byte PCIe reads and half the pinned memory.  The
 * slot arrays on the device stay float32 (hgs_resid_fetch_half) or hold the halves as they arrive
 * (hgs_resid_fetch_half_slots); the host side and the bus carry halves.  Eight 16-byte chunks:
 *   bytes   0 ..  95   48 halves: SH coefficients [0, 3 M) in the slot array's order, the rest padding
 *   bytes  96 .. 103   rotation, 4 halves
 *   bytes 104 .. 109   scale, 3 halves (activated, as the float rows hold it)
 *   bytes 110 .. 111   opacity, 1 half
 *   bytes 112 .. 123   mean, 3 float32 (never narrowed: scene coordinates need the mantissa)
 *   bytes 124 .. 127   padding
 * Narrowing rule, wherever this library turns a float into a half (hgs_resid_pack_rows, hgs_hier_write with
 * HGS_HIER_UPSTREAM_HALF, hgs.residency.pack_rows_half): round to nearest even, subnormal halves kept; a FINITE value
 * beyond +-65504 becomes +-65504 -- narrowing never makes an infinity (an infinite SH coefficient would turn into NaN
 * pixels); NaN stays NaN (the quiet NaN 0x7e00 under its sign) and an infinity stays an infinity.  Widening is exact.
 *   hgs_resid_fetch_half  hgs_resid_fetch on rows of this layout: same arguments, refusals and slot assignment; the
 *                         kernel reads the half rows over PCIe and widens them into the float slot arrays.
 *   hgs_resid_fetch_half_slots  the same call for half SLOTS (hgs_resid_rows_half): arguments, refusals and slot
 *                         assignment are those of hgs_resid_fetch_half, but the slot arrays hold SH, rotation, scale and
 *                         opacity as IEEE half and the mean as float32 -- the BITS of the host row are copied, nothing
 *                         is converted.  A slot costs 6 M + 28 bytes instead of 4 (3 M + 11): 124 against 236 at M = 16,
 *                         so a budget buys 1.90 times the rows.  No store touches a byte outside the assigned slot of
 *                         any array (16-byte stores into the SH rows only when 6 M % 16 == 0 and the array is 16-byte
 *                         aligned).  Alignment asked of the slot arrays: rotations 8 bytes, means3D 4, the others 2.
 *                         The rasterizer reads such slots with hgs_raster_args.lod_half_rows = 1.
 *   hgs_resid_pack_rows   device attribute arrays (`src`, G rows, activated) -> packed host rows, written by the kernel
 *                         through the mapped pointer: `half` = 1 this layout, 0 the float layout of
 *                         HGS_RESID_HOST_ROW_FLOATS; padding is written as zeros in both.  host_rows_packed: G rows
 *                         from hgs_host_alloc.  Ordered on `stream`: the host may read the rows once it has waited for
 *                         the stream.  G = 0 returns without a HIP call. */
#define HGS_RESID_HOST_ROW_BYTES_HALF 128
int hgs_resid_fetch_half(const int32_t* miss_ids, uint32_t m, const int32_t* free_list, uint32_t free_top, int32_t* slot_of,
                         int32_t* id_of_slot, uint32_t* stamp, uint32_t frame, const void* host_rows_packed,
                         const hgs_resid_rows* slot_rows, int32_t M, hgs_stream_t stream, int device);
typedef struct hgs_resid_rows_half {   /* the order of hgs_resid_rows */
  void* means3D;    /* float32 [rows, 3]    */
  void* shs;        /* half    [rows, M, 3] */
  void* opacities;  /* half    [rows]       */
  void* scales;     /* half    [rows, 3]    */
  void* rotations;  /* half    [rows, 4]    */
} hgs_resid_rows_half;
int hgs_resid_fetch_half_slots(const int32_t* miss_ids, uint32_t m, const int32_t* free_list, uint32_t free_top,
                               int32_t* slot_of, int32_t* id_of_slot, uint32_t* stamp, uint32_t frame,
                               const void* host_rows_packed, const hgs_resid_rows_half* slot_rows, int32_t M,
                               hgs_stream_t stream, int device);
int hgs_resid_pack_rows(const hgs_resid_rows* src, int64_t G, int32_t M, int32_t half, void* host_rows_packed,
                        hgs_stream_t stream, int device);

/* ---------------------------------------------------------------------------
 * A surface from depth maps (csrc/tsdf.hip; the rules, once for host and device, in csrc/tsdf_rule.h; the spec is
 * tests/tsdf_spec.py; hgs/meshing.py is the Python side): per-view depth maps -- hgs_raster_pixels' median_depth -- are
 * fused into a truncated signed distance volume, and a triangle mesh is extracted from it by naive surface nets.
 * Everything is float32 in a fixed operation order: the numpy restatement matches bit for bit.
 *
 * The volume: samples on the lattice x_a = lo_a + voxel * i_a, x fastest; tsdf [nz,ny,nx] in units of `trunc` (created
 * as 1), weight [nz,ny,nx] (created as 0), colour [nz,ny,nx,3] (created as 0) or NULL.  A view: planar depth [H,W]
 * (<= 0 or NaN: no surface at the pixel), weight [H,W] or NULL (1 everywhere), rgb [3,H,W] or NULL, the camera a centred
 * pinhole: view[3 r + c] = world_view_transform[r][c] (row vectors, as the rasterizer takes it), r < 4, c < 3.
 *   hgs_tsdf_integrate     applies views[0 .. n_views) in array order to every sample one of them sees: one call with V
 *                          views leaves the bits of V calls with one view each.  One pass over the volume, asynchronous
 *                          on `stream`; samples no view sees are neither read nor written.
 *   hgs_tsdf_extract_plan  marks the active cells (8 samples with weight >= min_weight whose tsdf differ in sign), counts
 *                          the quads, scans; waits once: totals_host[0] = vertices, totals_host[1] = quads (two
 *                          triangles each).  tmp: hgs_tsdf_extract_tmp_bytes(nx, ny, nz) bytes, 256-byte aligned.
 *   hgs_tsdf_extract_apply behind a successful plan on the same (device, tmp, dimensions) and an unchanged volume:
 *                          vertices [V,3], normals [V,3] (unit, towards free space; 0 for a zero gradient), colours [V,3]
 *                          or NULL, faces [2 Q,3]; vertices by ascending cell index, faces by ascending index of the
 *                          edge's lower sample, then axis.  Asynchronous; with V = 0 nothing is written.
 * Refused with HGS_ERR_INVALID before any HIP call (hgs_last_error names it): n_views outside 1..8; a dimension < 1 or
 * more than 2^31 - 1 samples (an extraction: more than (2^32 - 1) / 3, the quad offsets are 32-bit -- the size query then
 * answers 0); voxel, trunc or min_weight not positive and finite; max_weight <= 0 (infinity: never binds); W or H < 1 or more than 2^31 - 1 pixels; a
 * null tsdf, weight, depth, tmp, vertices, normals or faces; rgb without colour; colours without colour; a pointer that
 * is not 4-byte aligned, tmp not 256-byte aligned; apply without such a plan.
 * ------------------------------------------------------------------------- */
typedef struct hgs_tsdf_volume {
  float* tsdf;
  float* weight;
  float* colour; /* or NULL */
  float lo[3];
  float voxel;
  int32_t nx, ny, nz;
  float trunc;
  float max_weight;
} hgs_tsdf_volume;
typedef struct hgs_tsdf_view {
  const float* depth;
  const float* weight; /* or NULL */
  const float* rgb;    /* or NULL */
  int32_t W, H;
  float view[12];
  float tanfovx, tanfovy, z_min;
} hgs_tsdf_view;
int hgs_tsdf_integrate(const hgs_tsdf_volume* volume, const hgs_tsdf_view* views, int32_t n_views, hgs_stream_t stream,
                       int device);
size_t hgs_tsdf_extract_tmp_bytes(int32_t nx, int32_t ny, int32_t nz);
int hgs_tsdf_extract_plan(const hgs_tsdf_volume* volume, float min_weight, void* tmp, int64_t totals_host[2],
                          hgs_stream_t stream, int device);
int hgs_tsdf_extract_apply(const hgs_tsdf_volume* volume, const void* tmp, float* vertices, float* normals,
                           float* colours /* or NULL */, int32_t* faces, hgs_stream_t stream, int device);

/* ---------------------------------------------------------------------------
 * The same on a SPARSE volume (csrc/tsdf_sparse.hip; the allocation rule, once for host and device, in
 * csrc/tsdf_block_rule.h; the spec is tests/tsdf_sparse_spec.py): the lattice of
 * hgs_tsdf_volume is virtual -- a dimension may be anything up to 2^31 - 1 and the sample count anything --, storage is
 * 8 x 8 x 8 blocks near the observed surface: tsdf [B,8,8,8], weight [B,8,8,8], colour [B,8,8,8,3] or NULL (created as
 * 1 / 0 / 0 by the caller), block_of_slot int32 [B].  Block (bi, bj, bk) holds the samples 8 b .. 8 b + 7 per axis; the
 * block grid is ceil(n / 8) per axis, x fastest, at most 2^31 - 1 blocks.  `table` is ONE allocation, created as 0 by
 * the caller, dense over the block grid: hgs_tsdf_sparse_table_layout answers layout[0] = G blocks, slots int32 [G] at
 * byte 0 (-1: none, final after the commit), marks uint8 [G] at byte layout[1], a refusal word at byte layout[2],
 * layout[3] bytes in all.  n_blocks is -1 until the commit; afterwards the caller sets it to B.  On every lattice a dense
 * volume can hold, views marked, committed and then integrated leave the bits of hgs_tsdf_integrate in every allocated
 * sample, and the mesh is that of hgs_tsdf_extract_* in another order.
 *   hgs_tsdf_sparse_table_layout, _commit_tmp_bytes, _extract_tmp_bytes   need no GPU; the byte counts are 0 for sizes that
 *                          are refused.
 *   hgs_tsdf_sparse_mark   marks the blocks that the bands of views[0 .. n_views)'s pixels pass through (depth and weight
 *                          are read, rgb is not; a point up to one block outside the grid marks the border block next
 *                          to it): plain stores, accumulating over calls.  Asynchronous.
 *   hgs_tsdf_sparse_commit_plan   dilates the marks by the 3 x 3 x 3 block neighbourhood, counts, scans; waits once:
 *                          *n_blocks_host = B.  tmp: hgs_tsdf_sparse_commit_tmp_bytes bytes, 256-byte aligned.
 *   hgs_tsdf_sparse_commit_apply  with n_blocks = B and block_of_slot [capacity >= B], behind that plan on the same
 *                          (device, tmp): numbers the slots by ascending linear block index.  Asynchronous.
 *   hgs_tsdf_sparse_integrate     hgs_tsdf_integrate on the allocated blocks; a view that was not marked is legal and
 *                          updates the allocated blocks only.  Asynchronous.
 *   hgs_tsdf_sparse_extract_plan / _apply   as hgs_tsdf_extract_*; a cell or quad that needs a sample beyond the lattice
 *                          or in no allocated block is not emitted; vertices by (slot, place of the cell in its block,
 *                          64 k + 8 j + i), faces by (slot, place of the edge's lower sample, axis); cells int32 [V,3] =
 *                          the lattice cell of every vertex.  tmp: hgs_tsdf_sparse_extract_tmp_bytes(n_blocks) bytes.
 *                          With B = 0 nothing is launched or written.
 * Refused with HGS_ERR_INVALID before any HIP call (hgs_last_error names it): what hgs_tsdf_* refuses (the sample limits
 * apart); a block grid of more than 2^31 - 1 blocks; more than (2^32 - 1) / 3 / 512 blocks in an extraction; a null or
 * misaligned table or tmp (256 bytes); tsdf / weight / colour not 16-byte aligned; a mark or commit plan of a committed
 * volume (n_blocks != -1); commit apply, integrate or extract of one that is not (n_blocks < 0); capacity < n_blocks;
 * a marked view whose tanfovx or tanfovy is not in (0, 1.5]; trunc of more than 4096 voxels; an apply without its plan.
 * Refused by hgs_tsdf_sparse_commit_plan after its wait: a marked pixel whose footprint at d + trunc is more than
 * 16 x 2 voxels wide ("sub-pixel grid").  That pixel was not marched and the refusal word stays set, so this table can
 * never be committed: start again from a zeroed table, with a larger voxel or without that view.
 * ------------------------------------------------------------------------- */
typedef struct hgs_tsdf_sparse {
  float* tsdf;            /* [capacity,8,8,8] */
  float* weight;          /* [capacity,8,8,8] */
  float* colour;          /* [capacity,8,8,8,3] or NULL */
  int32_t* block_of_slot; /* [capacity] */
  void* table;
  float lo[3];
  float voxel;
  int32_t nx, ny, nz;
  float trunc;
  float max_weight;
  int32_t n_blocks;       /* -1 before the commit, B after it */
  int32_t capacity;       /* blocks the slot arrays have room for */
} hgs_tsdf_sparse;
int hgs_tsdf_sparse_table_layout(int32_t nx, int32_t ny, int32_t nz, int64_t layout[4]);
size_t hgs_tsdf_sparse_commit_tmp_bytes(int32_t nx, int32_t ny, int32_t nz);
size_t hgs_tsdf_sparse_extract_tmp_bytes(int32_t n_blocks);
int hgs_tsdf_sparse_mark(const hgs_tsdf_sparse* volume, const hgs_tsdf_view* views, int32_t n_views, hgs_stream_t stream,
                         int device);
int hgs_tsdf_sparse_commit_plan(const hgs_tsdf_sparse* volume, void* tmp, int64_t* n_blocks_host, hgs_stream_t stream,
                                int device);
int hgs_tsdf_sparse_commit_apply(const hgs_tsdf_sparse* volume, const void* tmp, hgs_stream_t stream, int device);
int hgs_tsdf_sparse_integrate(const hgs_tsdf_sparse* volume, const hgs_tsdf_view* views, int32_t n_views,
                              hgs_stream_t stream, int device);
int hgs_tsdf_sparse_extract_plan(const hgs_tsdf_sparse* volume, float min_weight, void* tmp, int64_t totals_host[2],
                                 hgs_stream_t stream, int device);
int hgs_tsdf_sparse_extract_apply(const hgs_tsdf_sparse* volume, const void* tmp, float* vertices, float* normals,
                                  float* colours /* or NULL */, int32_t* faces, int32_t* cells, hgs_stream_t stream,
                                  int device);

#ifdef __cplusplus
}
#endif
#endif /* HGS_H */
