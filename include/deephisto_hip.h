/* deephisto_hip.h -- C ABI of libdeephisto_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for the deephisto whole-slide patch hot path
 * (patch_samplers.full_samplers.FullImageDenseSampler ->
 *  examples.predict_full_patched.{batch_predictor, ImagePredictorPatched} ->
 *  models.patch_cls_simple.model.get_model).  The reference is pure Python and
 * has no FFI of its own; each entry point below names
 * the reference lines whose work it replaces, and INTEGRATION.md shows the
 * ctypes stub a reference maintainer would add at that line.
 *
 * Conventions
 *   - every function returns 0 on success or a negative DH_E* code; the text of
 *     the last failure on the calling thread is dh_last_error();
 *   - "dev" pointers are device (HBM) addresses owned by the caller, "host"
 *     pointers are ordinary host memory; nothing is retained past the call
 *     unless stated;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); device
 *     work is enqueued, never synchronised, unless stated;
 *   - no torch types, no C++ types: plain pointers and sizes only.
 */
#ifndef DEEPHISTO_HIP_H
#define DEEPHISTO_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DH_OK 0
#define DH_EINVAL (-22)  /* bad argument (shape, alignment, null pointer) */
#define DH_ENOMEM (-12)  /* device or host allocation failed */
#define DH_EHIP (-5)     /* a HIP runtime call or kernel launch failed */
#define DH_ENOSYS (-38)  /* entry point not available in this build */

/* layouts / dtypes of gathered tiles */
#define DH_LAYOUT_NHWC 0 /* [n, P, P, 3]  (FullImageDenseSampler.generator_torch) */
#define DH_LAYOUT_NCHW 1 /* [n, 3, P, P]  (batch_predictor's model input)          */
#define DH_DTYPE_F32 0
#define DH_DTYPE_BF16 1

int dh_abi_version(void);
const char* dh_last_error(void);

/* ---- a1: tile-origin grid (host, integer) -------------------------------
 * Replaces FullImageDenseSampler._create_batched_coords,
 * patch_samplers/full_samplers.py:374-404.  Order: interior grid (y-major) over
 * range(0,h-P,S) x range(0,w-P,S), last column, last row, corner; then the list
 * is padded with copies of the corner up to a multiple of `batch`.
 * dh_tile_grid_count: *n_unique = origins before padding, *n_padded = after.
 * dh_tile_grid: writes n_padded (y,x) int32 pairs to host memory out_yx. */
int dh_tile_grid_count(int64_t h, int64_t w, int32_t patch, int32_t stride, int32_t batch,
                       int64_t* n_unique, int64_t* n_padded);
int dh_tile_grid(int64_t h, int64_t w, int32_t patch, int32_t stride, int32_t batch,
                 int32_t* out_yx_host, int64_t capacity_pairs);

/* ---- synthetic slide (device) -------------------------------------------
 * Fills slide_dev[h][w][3] (uint8, HWC, row pitch w*3) with the closed-form
 * benchmark slide (formula frozen in oracle/synth.py / DESIGN.md).  The reference
 * reads real slides via psimage (full_samplers.py:328-330); this is bench input. */
int dh_synth_slide(uint8_t* slide_dev, int64_t h, int64_t w, uint32_t seed, void* stream);

/* ---- a2/a4/a5: tile gather + /255 + layout --------------------------------
 * Replaces _generate_batch_memory (full_samplers.py:353-369) + the feature
 * build of generator_torch (full_samplers.py:441-443; NHWC f32) or of
 * batch_predictor (examples/predict_full_patched.py:67-71; NCHW f32).
 * slide_dev: uint8[h][w][3]; yx_dev: int32[n][2] (y,x) origins on device;
 * out_dev: n*P*P*3 elements of `dtype` in `layout`.  Values are exactly
 * float32(k)/255 (bit-exact with NumPy), rounded to nearest-even for bf16.
 * Origins must satisfy 0 <= y <= h-P, 0 <= x <= w-P (checked on host only when
 * yx_host_check != NULL, which must then hold the same n pairs). */
int dh_tile_gather(const uint8_t* slide_dev, int64_t h, int64_t w, const int32_t* yx_dev,
                   const int32_t* yx_host_check, int64_t n, int32_t patch, int32_t layout,
                   int32_t dtype, void* out_dev, void* stream);

/* Same gather with the batch-level augmentation of the training pipeline fused in
 * (models/patch_cls_simple/train.py:71-81: permute to NCHW, then RandomHorizontalFlip /
 * RandomVerticalFlip applied to the whole batch, i.e. one coin per batch): flip_h mirrors
 * columns, flip_v mirrors rows of every tile.  Feeds the a9 output contract
 * (patch_samplers/region_samplers.py:616-621, 729-738).  Origins may lie partly or wholly outside the
 * slide (the region samplers' origin bounds, region_samplers.py:112-118, allow a patch to hang over the
 * border): pixels outside [0,h) x [0,w) are written as 0, nothing outside the slide is read. */
int dh_tile_gather_aug(const uint8_t* slide_dev, int64_t h, int64_t w, const int32_t* yx_dev,
                       int64_t n, int32_t patch, int32_t layout, int32_t dtype, int32_t flip_h,
                       int32_t flip_v, void* out_dev, void* stream);

/* dh_tile_gather_aug with a per-tile stain jitter fused in (no counterpart in the
 * reference).  A source pixel inside the slide goes T_c = od[byte_c]; o_c = A[c][0] T_r + A[c][1] T_g +
 * A[c][2] T_b + b_c in 64-bit integers; v'_c = lut_dev[clamp(o_c >> shift, 0, lut_n - 1)]; the output is
 * float32(v'_c) / 255, correctly rounded, then rounded to nearest-even for bf16.  Pixels outside the slide are
 * written as 0 and are not transformed.  params_dev: int32[n][12], per tile the matrix A row-major
 * (|.| <= 2^19) then the bias b (|.| <= 2^30); params_host_check: the same values on the host, every one
 * checked before the launch, or NULL.  od_dev / od_host, lut_dev (16-byte aligned) / lut_n <= 24576 and shift
 * in [0, 40) as for dh_stain_apply.  Integer work up to the final division: the result is the same bits
 * wherever it runs. */
int dh_tile_gather_stain_aug(const uint8_t* slide_dev, int64_t h, int64_t w, const int32_t* yx_dev,
                             const int32_t* params_dev, const int32_t* params_host_check, int64_t n, int32_t patch,
                             int32_t layout, int32_t dtype, int32_t flip_h, int32_t flip_v, const int32_t* od_dev,
                             const int32_t* od_host, int32_t shift, const uint8_t* lut_dev, int32_t lut_n,
                             void* out_dev, void* stream);

/* dh_tile_gather_aug with a per-tile rotation and scale about the patch centre fused in, and optionally the
 * stain jitter above (no counterpart in the reference).  affine_dev: int32[n][4], per
 * tile m = round(2^15 s [[cos, -sin], [sin, cos]]) row-major, s = source pixels per output pixel (|.| <= 2^16);
 * affine_host_check: the same values on the host, every one checked before the launch, or NULL.  With (sr, sx)
 * the flipped row and column of an output pixel, U2 = 2 sx + 1 - patch, V2 = 2 sr + 1 - patch, the source
 * point in Q16 is X = ((2 x0 + patch) << 15) - 2^15 + m00 U2 + m01 V2, Y likewise from y0, m10, m11 (64-bit);
 * taps (X >> 16, Y >> 16) and its three neighbours, weights fx = (X >> 8) & 255, fy likewise, a tap outside
 * the slide reads as 0; per channel v = ((a (256 - fx) + b fx)(256 - fy) + (c (256 - fx) + d fx) fy + 2^15) >> 16.
 * v then goes where the slide byte goes in the entries above: float32(v) / 255, or, with the stain arguments,
 * through od, matrix, bias and lut first.  params_dev, od_dev, od_host and lut_dev are all given or all NULL
 * (NULL: no stain jitter; params_host_check, shift and lut_n are then unused).  A pixel none of whose taps of
 * non-zero weight lies inside the slide is written as 0 and is not transformed.  patch in [1, 4096].  The
 * identity row (32768, 0, 0, 32768) gives the bits of dh_tile_gather_aug / dh_tile_gather_stain_aug. */
int dh_tile_gather_affine_aug(const uint8_t* slide_dev, int64_t h, int64_t w, const int32_t* yx_dev,
                              const int32_t* params_dev, const int32_t* params_host_check, const int32_t* affine_dev,
                              const int32_t* affine_host_check, int64_t n, int32_t patch, int32_t layout,
                              int32_t dtype, int32_t flip_h, int32_t flip_v, const int32_t* od_dev,
                              const int32_t* od_host, int32_t shift, const uint8_t* lut_dev, int32_t lut_n,
                              void* out_dev, void* stream);

/* FullImageRndSampler.generator_torch (full_samplers.py:277-290) stacks the uint8 patches into a
 * float tensor WITHOUT dividing by 255: float32[n][P][P][3] with values 0..255 (0 outside the slide). */
int dh_tile_gather_raw(const uint8_t* slide_dev, int64_t h, int64_t w, const int32_t* yx_dev,
                       int64_t n, int32_t patch, float* out_dev, void* stream);

/* coords tensor of generator_torch (full_samplers.py:444-451): float32[n][2]. */
int dh_tile_coords_f32(const int32_t* yx_dev, int64_t n, float* out_dev, void* stream);

/* ---- a8: logit accumulation + argmax ------------------------------------
 * Replaces the per-patch `prediction[y//d:(y+P)//d, x//d:(x+P)//d, :] += logits[i]`
 * loop and the final argmax of ImagePredictorPatched.process
 * (examples/predict_full_patched.py:41-62).  Tiles are applied in list order
 * (duplicates included) with one float32 add each, so the canvas is bit-exact
 * with NumPy for identical logits.  yx_host: int32[n][2] host copy of origins;
 * logits_dev: float32[n][n_cls]; canvas_dev: float32[dh][dw][n_cls] (accumulated
 * into -- zero it first for a fresh prediction), dh = h/d, dw = w/d (floor).
 * map_dev (optional, may be NULL): int64[dh][dw] = first index of the maximum
 * over classes of the updated canvas (NumPy argmax tie/NaN rule).
 * The per-bin tile lists built from yx_host are cached per thread and reused while the same
 * origins are passed again (whole-slide prediction repeats one grid): such calls are fully
 * asynchronous; a call with new origins synchronises the stream once. */
int dh_accumulate_logits(const float* logits_dev, const int32_t* yx_host, int64_t n,
                         int32_t patch, int32_t downscale, int32_t n_cls, int64_t h, int64_t w,
                         float* canvas_dev, int64_t* map_dev, void* stream);
int dh_argmax_map(const float* canvas_dev, int64_t n_cells, int32_t n_cls, int64_t* map_dev,
                  void* stream);

/* ---- e1: the exchange step of the tile-sharded prediction -------------------------------
 * The reference predicts every tile on one device and sums the logits into the canvas in list order
 * (examples/predict_full_patched.py:40-63).  Sharded over ranks each rank predicts a
 * contiguous range of that list; this call is the ONE exchange: every rank contributes
 * float32[n_per_rank][n_cls] (ranges padded to a common length by the caller) and receives
 * float32[world][n_per_rank][n_cls] in rank order, after which each rank runs dh_accumulate_logits on the
 * whole list.  comm: the caller's RCCL communicator (ncclComm_t), created by the caller with the RCCL of
 * its process.  The ncclAllGather that runs must belong to the SAME library instance that made `comm`: this
 * library never links against or loads an RCCL of its own.  dh_set_rccl(handle) hands over the dlopen handle of
 * the host's RCCL (exact; NULL = back to automatic); without it the first exchange takes DH_RCCL_LIB=<file>
 * (must already be loaded), else a global ncclAllGather symbol, else an already-loaded librccl.so.1 / librccl.so;
 * nothing loaded => DH_EINVAL.  Asynchronous on `stream`.  The Python shims exchange through torch.distributed
 * instead (examples/predict_full_patched.py: exchange_logits). */
int dh_set_rccl(void* dl_handle);
int dh_allgather_logits(void* comm, const float* send_dev, float* recv_dev, int64_t n_per_rank,
                        int32_t n_cls, void* stream);

/* ---- visualisation of the class map (examples/predict_full_patched.py:81-113) ----
 * dh_colorize_map: `colored[pred == anno.id] = anno.color` for every class (:93-95):
 *   rgb[i] = lut[map[i]] when 0 <= map[i] < n_cls, else (0,0,0); lut = uint8[n_cls][3] on the device.
 * dh_overlay_blend: `(img * alpha + colored * (1 - alpha)).astype(np.uint8)` (:109-110) in float64,
 *   truncating like NumPy's cast; n_bytes = h*w*3. */
int dh_colorize_map(const int64_t* map_dev, int64_t n_cells, const uint8_t* lut_dev, int32_t n_cls,
                    uint8_t* rgb_dev, void* stream);
int dh_overlay_blend(const uint8_t* img_dev, const uint8_t* colored_dev, int64_t n_bytes, double alpha,
                     uint8_t* out_dev, void* stream);

/* ---- whole-slide probability maps ---------------------------------
 * The `count` array and the `prediction /= count` line that examples/predict_full_patched.py:45, 55-58, 61 carry commented
 * out, over per-tile softmax probabilities instead of raw logits.  All float32; tile list, footprints
 * (rows y/d .. (y+P)/d, columns x/d .. (x+P)/d, clipped) and order are those of dh_accumulate_logits, one writer per cell,
 * no atomics: every output is bit-identical to the sequential NumPy loop.
 * dh_softmax_rows: probs[i][c] = e_c / s with m = max_c x_c, e_c = expf(x_c - m), s = e_0 + e_1 + ... in class order;
 *   logits_dev, probs_dev: float32[n][n_cls], n_cls <= 64; probs_dev may be logits_dev.
 * dh_accumulate_mean: sum_dev[cell][:] += probs[t][:] and count_dev[cell] += 1 for every tile t covering the cell, in list
 *   order (duplicates included).  sum_dev float32[dh][dw][n_cls] and count_dev int32[dh][dw] are accumulated into (zero both
 *   for a fresh slide), so runs of different patch size chain.  map_dev / confidence_dev (both or neither, may be NULL):
 *   when given, the finish below runs in the same pass, in place: sum_dev then holds the probabilities.  Shares the cached
 *   bin plan of dh_accumulate_logits (the same origins right after it cost no rebuild).  n = 0 is allowed.
 * dh_finish_mean: where count > 0: proba = sum / float32(count), map = first index of the maximum of proba (NumPy argmax
 *   tie/NaN rule), confidence = proba[map]; where count == 0: proba = 0, confidence = 0, map = fill_class.
 *   proba_dev may be sum_dev.  map_dev int64[n_cells], confidence_dev float32[n_cells].
 * dh_heatmap_blend: out[i][c] = uint8(img[i][c] * alpha + (float64(field[i * field_stride]) * color[c]) * (1 - alpha)) in
 *   float64, truncating like NumPy's cast; img_dev, out_dev: uint8[n_cells][3]; field_dev: float32, one value per cell,
 *   field_stride elements apart (n_cls for one class of the probabilities, 1 for the confidence); color_host: uint8[3]. */
int dh_softmax_rows(const float* logits_dev, int64_t n, int32_t n_cls, float* probs_dev, void* stream);
int dh_accumulate_mean(const float* probs_dev, const int32_t* yx_host, int64_t n, int32_t patch, int32_t downscale,
                       int32_t n_cls, int64_t h, int64_t w, float* sum_dev, int32_t* count_dev, int64_t* map_dev,
                       float* confidence_dev, int32_t fill_class, void* stream);
int dh_finish_mean(const float* sum_dev, const int32_t* count_dev, int64_t n_cells, int32_t n_cls, int32_t fill_class,
                   float* proba_dev, int64_t* map_dev, float* confidence_dev, void* stream);
int dh_heatmap_blend(const uint8_t* img_dev, const float* field_dev, int64_t field_stride, int64_t n_cells,
                     const uint8_t* color_host, double alpha, uint8_t* out_dev, void* stream);

/* ---- scoring a class map against a polygon annotation (no counterpart in the reference) --------
 * dh_rasterize_regions: labels_dev int32[dh][dw] from n_rings polygon rings.  xy_host float64[n_vertices][2] (x, y) in layer
 *   coordinates; ring r owns the vertices ring_start_host[r] .. ring_start_host[r + 1] (int64[n_rings + 1], first entry 0; the
 *   closing edge last -> first is implied) and has class ring_class_host[r] in [0, n_cls), n_cls <= 64.  Cell (cy, cx) is its
 *   centre p = ((cx + 0.5) * d, (cy + 0.5) * d).  p is inside a ring when an odd number of its edges a -> b have
 *   (a.y > p.y) != (b.y > p.y) and p.x < a.x + (p.y - a.y) * (b.x - a.x) / (b.y - a.y), evaluated in float64 in that order,
 *   one rounding per operation.  A cell inside rings of exactly one class gets that class id; of none, or of several
 *   different classes, -1.  n_rings = 0 gives all -1.  A ring with fewer than 3 vertices, a class id outside [0, n_cls), a
 *   coordinate that is not finite (or beyond 1e15), n_cls > 64 and non-positive dh / dw / d are refused before any GPU call.
 *   The ring data and the per-bin ring lists stay on the device for the next call with the same arguments.
 * dh_confusion_matrix: counts_host int64[n_cls][n_cls + 1], HOST memory: counts[t][p] = cells with truth t and prediction p;
 *   the last column counts cells with truth t and prediction -1 (no prediction).  Cells with truth -1 are not counted.
 *   pred_dev int64[n_cells], truth_dev int32[n_cells]; outcome_dev int64[n_cells] or NULL: -1 where truth is -1, 0 where
 *   the prediction equals the truth, 1 elsewhere.  The entry waits for the stream: a prediction outside [-1, n_cls)
 *   anywhere in pred_dev makes it return DH_EINVAL (counts_host is then all zero). */
int dh_rasterize_regions(const double* xy_host, const int64_t* ring_start_host, const int32_t* ring_class_host, int64_t n_rings,
                         int32_t n_cls, int64_t dh, int64_t dw, int32_t d, int32_t* labels_dev, void* stream);
int dh_confusion_matrix(const int64_t* pred_dev, const int32_t* truth_dev, int64_t n_cells, int32_t n_cls, int64_t* counts_host,
                        int64_t* outcome_dev, void* stream);

/* ---- regions of a class map: connected components, table, cleanup (no counterpart in the reference) --
 * dh_label_components: labels_dev int32[dh][dw] from map_dev int64[dh][dw] with values in [-1, n_cls), n_cls <= 64, fewer than
 *   2^31 - 2048 cells.  Two cells belong to one component when they have the same class >= 0 and a path of 4-neighbours of that
 *   class joins them.  labels is 0 where the class is -1, else the component's id in 1..K, ids ascending with the component's
 *   smallest linear cell index cy * dw + cx: the numbering is unique.  work_dev: int32[dh_label_work_size(dh * dw)], scratch.
 *   *n_components_host = K.  The entry waits for the stream; a class outside [-1, n_cls) anywhere in map_dev makes it return
 *   DH_EINVAL (labels_dev is then undefined).
 * dh_label_work_size: the number of int32 elements of work_dev for a canvas of n_cells cells.
 * dh_region_stats: table_dev int64[n_components][10], one row per id (row id - 1), all integers, so exact whatever the order:
 *   0 class, 1 area in cells, 2..5 bounding box y0, x0, y1, x1 in cells (half-open), 6 sum of cy, 7 sum of cx, 8 the smallest
 *   linear cell index, 9 conf_q = the sum over the cells, modulo 2^64, of rint(float64(confidence) * 2^32) (round half to
 *   even); 0 when confidence_dev (float32[dh][dw]) is NULL.  labels_dev and n_components as dh_label_components gave them for
 *   map_dev.  Asynchronous on the stream.
 * dh_clean_small_regions: one cleanup round.  A component is small when its area < min_cells (>= 1).  Every pair (cell of a
 *   small component s, 4-neighbour cell in a component that is not small) casts one vote for the neighbour's class; s takes
 *   the class with the most votes, the lowest class id on a tie, and stays as it is without a vote.  All small components are
 *   decided from the one labelling, then out_map_dev int64[dh][dw] (not map_dev) = the map with them rewritten; cells of
 *   class -1 neither vote nor change.  votes_dev: int32[n_components][n_cls], scratch.  *n_changed_host = cells whose class
 *   changed; the entry waits for the stream. */
int dh_label_components(const int64_t* map_dev, int64_t dh, int64_t dw, int32_t n_cls, int32_t* labels_dev, int32_t* work_dev,
                        int64_t* n_components_host, void* stream);
int64_t dh_label_work_size(int64_t n_cells);
int dh_region_stats(const int64_t* map_dev, const int32_t* labels_dev, const float* confidence_dev, int64_t dh, int64_t dw,
                    int64_t n_components, int64_t* table_dev, void* stream);
int dh_clean_small_regions(const int64_t* map_dev, const int32_t* labels_dev, const int64_t* table_dev, int64_t n_components,
                           int64_t dh, int64_t dw, int32_t n_cls, int64_t min_cells, int32_t* votes_dev, int64_t* out_map_dev,
                           int64_t* n_changed_host, void* stream);

/* ---- distance maps of a class map: class masks, exact Euclidean distance transform (no counterpart in
 * the reference) ----
 * dh_class_mask: mask_dev uint8[dh][dw] (0 / 1) from map_dev int64[dh][dw] with values in [-1, 63].  A cell is a member when its
 *   class k >= 0 has bit k of class_bits set, or when it is -1 and include_unclassified is not 0.  mode 0: the members.  mode 1:
 *   the members with at least one 4-neighbour inside the canvas that is not a member (the set's boundary; the canvas edge makes
 *   none).  mode 2: the cells with at least one 4-neighbour inside the canvas of a different value, -1 counting as a value
 *   (every label change; class_bits and include_unclassified are ignored).  dh, dw in [1, 32767].  The entry waits for the
 *   stream; a value outside [-1, 63] anywhere in map_dev makes it return DH_EINVAL (mask_dev is then undefined).
 * dh_distance_transform: d2_dev int32[dh][dw] = for every cell the minimum over the feature cells (mask != 0) of dy^2 + dx^2 in
 *   cells, exact; nearest_dev int32[dh][dw] (or NULL) = the linear index y' * dw + x' of the feature cell that attains it, the
 *   smallest index among equals.  Without a feature cell d2 = INT32_MAX and nearest = -1 everywhere.  dh, dw in [1, 32767]
 *   (2 * 32767^2 < 2^31).  work_dev: int32[dh_distance_work_size(dh, dw)], scratch.  Integer arithmetic only, no atomics: the
 *   result does not depend on the launch.  Asynchronous on the stream.
 * dh_distance_work_size: the number of int32 elements of work_dev; 0 for a canvas outside the limits. */
int dh_class_mask(const int64_t* map_dev, int64_t dh, int64_t dw, uint64_t class_bits, int32_t include_unclassified, int32_t mode,
                  uint8_t* mask_dev, void* stream);
int64_t dh_distance_work_size(int64_t dh, int64_t dw);
int dh_distance_transform(const uint8_t* mask_dev, int64_t dh, int64_t dw, int32_t* d2_dev, int32_t* nearest_dev, int32_t* work_dev,
                          void* stream);

/* ---- a6: ResNet-18 patch classifier forward ---------------------------------
 * Replaces `model(features)` for the network built by get_model
 * (models/patch_cls_simple/model.py:5-11: torchvision resnet18 + fc[n_cls,512])
 * in eval mode, as called from batch_predictor (predict_full_patched.py:77).
 * A handle owns device copies of the parameters (packed for MFMA) and the
 * activation workspace; one handle per thread/stream.
 * compute dtype: DH_DTYPE_F32 (f32 MFMA, logits within 1e-4 of the CPU path) or
 * DH_DTYPE_BF16 (bf16 MFMA, f32 accumulate). */
typedef struct dh_resnet18 dh_resnet18;
int dh_resnet18_create(dh_resnet18** out, int32_t n_classes, int32_t compute_dtype);
void dh_resnet18_destroy(dh_resnet18* net);
/* Set one parameter/buffer by its torchvision state_dict name ("conv1.weight",
 * "layer2.0.downsample.1.running_var", "fc.bias", ...).  data_host: float32,
 * n_elem must match.  "num_batches_tracked" entries are accepted and ignored. */
int dh_resnet18_set_param(dh_resnet18* net, const char* name, const float* data_host,
                          int64_t n_elem);
/* Call after all parameters are set (or changed): folds BN running stats into
 * per-channel scale/shift and packs conv weights into MFMA fragment order.
 * Checks all parameters before it uploads any. */
int dh_resnet18_finalize(dh_resnet18* net, void* stream);
/* x_dev: float32[n][3][P][P] NCHW in [0,1] (what batch_predictor feeds the model);
 * logits_dev: float32[n][n_classes].  P must be a multiple of 32. */
int dh_resnet18_forward(dh_resnet18* net, const float* x_dev, int64_t n, int32_t patch,
                        float* logits_dev, void* stream);
/* Fused a2+a5+a6: gathers the tiles straight from the uint8 slide inside the
 * stem kernel (no float copy of the pixels is ever written to HBM). */
int dh_resnet18_forward_tiles(dh_resnet18* net, const uint8_t* slide_dev, int64_t h, int64_t w,
                              const int32_t* yx_dev, int64_t n, int32_t patch,
                              float* logits_dev, void* stream);

/* ---- ResNet-50 patch classifier forward (bf16 inference) ------------------------------------
 * The same entry points for the network get_model(..., arch="resnet50") returns (torchvision resnet50 v1.5 +
 * fc[n_cls, 2048]), in eval mode: bf16 activations, bf16 MFMA with f32 accumulation, f32 logits.  finalize folds the
 * eval BN (running statistics) into the convolution weights and a per-channel bias; every convolution is then one
 * pass that writes its final activation (bias [+ identity], ReLU).  set_param takes torchvision state_dict names.
 * P: 64 <= P <= 256, P % 32 == 0.  At most DH_RESNET50_MAX_TILES tiles per call (the activation maps stay within 2^31
 * bytes); more is refused.  forward_tiles reads the n origins back and checks them against the slide (one
 * synchronisation of `stream`) before any launch.  Per-tile logits do not depend on the launch size. */
#define DH_RESNET50_MAX_TILES 1024
typedef struct dh_resnet50 dh_resnet50;
int dh_resnet50_create(dh_resnet50** out, int32_t n_classes);
void dh_resnet50_destroy(dh_resnet50* net);
int dh_resnet50_set_param(dh_resnet50* net, const char* name, const float* data_host, int64_t n_elem);
int dh_resnet50_finalize(dh_resnet50* net, void* stream);
int dh_resnet50_forward(dh_resnet50* net, const float* x_dev, int64_t n, int32_t patch, float* logits_dev,
                        void* stream);
int dh_resnet50_forward_tiles(dh_resnet50* net, const uint8_t* slide_dev, int64_t h, int64_t w,
                              const int32_t* yx_dev, int64_t n, int32_t patch, float* logits_dev,
                              void* stream);

/* ---- tile embeddings: the pooled features one step before the logits ----------
 * forward_tiles with the global average pool of every tile's last stored activation written out as well:
 * feat_dev[i][c] = mean over the pixels of channel c (torchvision's channel order), float32[n][512] for ResNet-18 and
 * float32[n][2048] for ResNet-50 (16-byte aligned there).  Summation order and the 1/HW multiply are those of the head of
 * forward_tiles, so logits_dev (float32[n][n_classes]) receives the bits forward_tiles writes; with logits_dev == NULL the
 * fc is skipped.  Every argument check of the forward_tiles sibling applies (patch, launch limits, origins). */
int dh_resnet18_features_tiles(dh_resnet18* net, const uint8_t* slide_dev, int64_t h, int64_t w,
                               const int32_t* yx_dev, int64_t n, int32_t patch, float* feat_dev,
                               float* logits_dev, void* stream);
int dh_resnet50_features_tiles(dh_resnet50* net, const uint8_t* slide_dev, int64_t h, int64_t w,
                               const int32_t* yx_dev, int64_t n, int32_t patch, float* feat_dev,
                               float* logits_dev, void* stream);

/* ---- class activation maps of the last conv: fine whole-slide maps ----------
 * Both engines end in global average pool + fc, so a tile's logits are the mean over the positions of its last activation of
 * fc applied at each position.  cam_tiles is forward_tiles with those per-position terms written out:
 *   cam_dev[t][p][k] = fc_b[k] + sum_c fc_w[k][c] * a[t][p][c],  float32[n][S * S][n_classes], S = patch / 32, p = i * S + j
 * with i along y and j along x; position (i, j) is the 32 x 32-pixel block of the tile at (32 i, 32 j).  float32 accumulation
 * in an order fixed by the engine and n_classes alone (not by n, the tile's index or S), no atomics.  patch % 32 == 0 and
 * n_classes <= 64, or DH_EINVAL; every argument check of the forward_tiles sibling applies as well.  logits_dev (may be NULL:
 * the pooling head is then not launched) receives the bits forward_tiles writes.
 * dh_accumulate_cam / dh_accumulate_cam_mean: dh_accumulate_logits / dh_accumulate_mean over the EXPANDED list, bit for bit,
 *   without building it: the expanded list has one entry of patch size 32 per tile and position, tile-major with positions in
 *   order p, at origin (y + 32 i, x + 32 j), with row cam_dev[t][p] (cam_mean: probs_dev[t][p], e.g. dh_softmax_rows over
 *   the n * S * S rows).  The sub-tiles' cell ranges partition the tile's, so a tile adds exactly one position to every cell
 *   it covers -- i = ceil(((cy + 1) d - y) / 32) - 1, likewise j -- and the order of additions in a cell is the tile order.
 *   yx_host, n, patch: the TILE list (int32[n][2]) and tile size, patch % 32 == 0; h, w <= 2^31 - 65; everything else as in
 *   dh_accumulate_logits / dh_accumulate_mean, whose cached bin plan these share. */
int dh_resnet18_cam_tiles(dh_resnet18* net, const uint8_t* slide_dev, int64_t h, int64_t w, const int32_t* yx_dev,
                          int64_t n, int32_t patch, float* cam_dev, float* logits_dev, void* stream);
int dh_resnet50_cam_tiles(dh_resnet50* net, const uint8_t* slide_dev, int64_t h, int64_t w, const int32_t* yx_dev,
                          int64_t n, int32_t patch, float* cam_dev, float* logits_dev, void* stream);
int dh_accumulate_cam(const float* cam_dev, const int32_t* yx_host, int64_t n, int32_t patch, int32_t downscale,
                      int32_t n_cls, int64_t h, int64_t w, float* canvas_dev, int64_t* map_dev, void* stream);
int dh_accumulate_cam_mean(const float* probs_dev, const int32_t* yx_host, int64_t n, int32_t patch, int32_t downscale,
                           int32_t n_cls, int64_t h, int64_t w, float* sum_dev, int32_t* count_dev, int64_t* map_dev,
                           float* confidence_dev, int32_t fill_class, void* stream);

/* ---- e2: embedding rows: normalise, prototype scores, per-class sums -----------
 * Row-major float32 on the device, no atomics.  A row's result depends on that row alone: not on n, not on the
 * row's place in the launch, not on the grid.  D % 64 == 0 and 64 <= D <= 4096, 1 <= K <= 64; float pointers are
 * 16-byte aligned.  Anything else is refused with DH_EINVAL and the argument's name in dh_last_error().  n = 0 is allowed.
 * dh_embed_normalize: out[i] = in[i] / sqrt(sum_c in[i][c]^2); a row whose sum of squares is 0 stays all zero.
 *   out_dev may be in_dev (in place); any other overlap is undefined.
 * dh_embed_scores: scores[i][k] = scale * sum_c feat[i][c] * proto[k][c], one fused multiply-add per c in ascending c
 *   from 0; proto_dev float32[K][D], scores_dev float32[n][K].
 * dh_embed_class_sums: sums_dev[k] (float32[K][D]) = the sum of the rows i with label_dev[i] == k (int32[n]; labels
 *   outside [0, K), -1 among them, are ignored), counts_dev[k] (int64[K]) their number.  The order is the contract:
 *   rows are cut into chunks of DH_EMBED_CHUNK_ROWS; a chunk's partial starts at 0 and adds its rows in ascending
 *   order; the result starts at 0 and adds the partials of ALL chunks in ascending chunk order (float32 throughout).
 *   work_dev: float32[dh_embed_class_work_size(n, D, K)] scratch (16-byte aligned); the size is -1 for bad arguments.
 * dh_embed_assign: per row i the nearest of the K rows of centres_dev (float32[K][D]):
 *   dist_dev[i] (float32[n]) the smallest squared Euclidean distance, label_dev[i] (int32[n]) = k0 + the index of the
 *   centre that attains it.  A distance is ONE accumulator from 0: for c ascending t = feat[i][c] - centre[k][c] (one
 *   float32 subtract), acc = fma(t, t, acc); so a row equal to a centre gets exactly 0.  The choice is the
 *   lexicographic minimum of (distance, index) from the start (+inf, -1): at equal distances the lower index wins, a
 *   NaN or +inf distance never does, and a row with no finite distance gets (-1, +inf).  merge != 0: the start is
 *   the row's existing (dist_dev[i], label_dev[i]) instead, which is kept at ties when its index is the lower (the
 *   caller's part); this assigns against more than 64 centres in passes (k0 = 0, 64, ...).  k0 >= 0.
 * dh_embed_scatter: scatter_dev (float32[D][D], both triangles written) = the scatter matrix of the
 *   rows about mean_dev (float32[D]): S[a][b] = sum_i t_i[a] * t_i[b] with t_i[c] = feat[i][c] - mean[c] (one float32
 *   subtract).  The order is the contract: rows are cut into chunks of DH_EMBED_CHUNK_ROWS; a chunk's partial is ONE
 *   accumulator from 0, for its rows in ascending order acc = fma(t[a], t[b], acc); the result starts at 0 and adds the
 *   partials of ALL chunks in ascending chunk order (float32 throughout).  Hence S[a][b] and S[b][a] are the same bits,
 *   the result does not depend on the grid, and n = 0 writes all zeros (into scatter_dev when it is given; no pointer
 *   is needed then).  work_dev: float32[dh_embed_scatter_work_size(n, D)] scratch (16-byte aligned; may be NULL when
 *   the size is 0); the size is -1 for bad arguments.
 * dh_embed_project: out[i][j] = scale[j] * acc for j < K with ONE accumulator from 0: for c
 *   ascending acc = fma(feat[i][c] - mean[c], comp[j][c], acc) (one float32 subtract).  comp_dev float32[K][D],
 *   scale_dev float32[K] or NULL (every scale 1), out_dev float32[n][ld] with K <= ld <= 4096 and ld % 4 == 0;
 *   columns K .. ld - 1 of out_dev are not touched.  A row's result depends on that row alone.
 * dh_embed_knn: for every row i of query_dev (float32[n][D]) the k nearest rows of bank_dev
 *   (float32[m][D]), exactly.  For query row i and bank row j the distance is that of dh_embed_assign: ONE accumulator from
 *   0, for c ascending t = q[c] - b[c] (one float32 subtract), acc = fma(t, t, acc).  Row i of index_dev (int32[n][k]) and
 *   dist_dev (float32[n][k]) holds the k smallest pairs under the lexicographic order (distance, m0 + j), stored ascending:
 *   a total order, so the result is one well-defined list however the bank is walked.  A NaN (or +inf) distance never
 *   enters; if fewer than k candidates are finite the tail is (-1, +inf).  merge != 0: the list already in index_dev /
 *   dist_dev (ascending, or the (-1, +inf) padding) counts as candidates too, so a bank larger than one call, or one held
 *   in several tensors, goes through in passes with rising m0 and the result is the bits of the single call.
 *   1 <= k <= 64; D as above; 0 <= m, 0 <= m0, m0 + m <= 2^31 - 1; both matrices 16-byte aligned, the outputs 4-byte
 *   aligned.  n == 0 is a no-op, m == 0 without merge fills the padding, m == 0 with merge changes nothing.  No atomics;
 *   a query row's output does not depend on n, on the row's place or on the other rows.
 * dh_embed_knn_votes: one vote per neighbour.  Row i walks index_dev[i][0 .. k) in stored order; an index of -1, an index
 *   outside [0, m) or a bank_label_dev (int32[m]) entry outside [0, n_classes) casts no vote.  votes_dev[i][c]
 *   (int32[n][n_classes]) are the counts, label_dev[i] (int32[n]) the class with the most votes; at equal votes the class
 *   whose first member comes earliest in the neighbour list (the nearer neighbour wins); -1 when nobody voted.
 *   1 <= k <= 64, 1 <= n_classes <= 64, 0 <= m <= 2^31 - 1. */
#define DH_EMBED_CHUNK_ROWS 1024
int dh_embed_normalize(const float* in_dev, int64_t n, int32_t D, float* out_dev, void* stream);
int dh_embed_scores(const float* feat_dev, int64_t n, int32_t D, const float* proto_dev, int32_t K, float scale,
                    float* scores_dev, void* stream);
int64_t dh_embed_class_work_size(int64_t n, int32_t D, int32_t K);
int dh_embed_class_sums(const float* feat_dev, const int32_t* label_dev, int64_t n, int32_t D, int32_t K,
                        float* sums_dev, int64_t* counts_dev, float* work_dev, void* stream);
int dh_embed_assign(const float* feat_dev, int64_t n, int32_t D, const float* centres_dev, int32_t K, int32_t k0,
                    int32_t merge, int32_t* label_dev, float* dist_dev, void* stream);
int64_t dh_embed_scatter_work_size(int64_t n, int32_t D);
int dh_embed_scatter(const float* feat_dev, int64_t n, int32_t D, const float* mean_dev, float* scatter_dev,
                     float* work_dev, void* stream);
int dh_embed_project(const float* feat_dev, int64_t n, int32_t D, const float* mean_dev, const float* comp_dev,
                     int32_t K, const float* scale_dev, float* out_dev, int32_t ld, void* stream);
int dh_embed_knn(const float* query_dev, int64_t n, const float* bank_dev, int64_t m, int32_t D, int32_t k, int64_t m0,
                 int32_t merge, int32_t* index_dev, float* dist_dev, void* stream);
int dh_embed_knn_votes(const int32_t* index_dev, int64_t n, int32_t k, const int32_t* bank_label_dev, int64_t m,
                       int32_t n_classes, int32_t* votes_dev, int32_t* label_dev, void* stream);

/* ---- a7: training step (float32) -------------------------------------------------------
 * Replaces, for the same network, models/patch_cls_simple/train.py:168-172:
 *   outputs = model(inputs); loss = criterion(outputs, labels); loss.backward(); optimizer.step()
 * with CrossEntropyLoss (mean) at train.py:117 and Adam(lr) at train.py:118 (PyTorch
 * defaults: betas (0.9, 0.999), eps 1e-8, no weight decay; BatchNorm momentum 0.1, eps 1e-5,
 * batch statistics, running statistics updated with the unbiased variance).
 * Training state (master parameters, gradients, Adam moments, running statistics, saved
 * activations; all in HBM) is created by the first dh_resnet18_forward_train / _train_begin
 * for a batch shape from the parameters set with dh_resnet18_set_param, and folded back into
 * the handle (for eval-mode forwards) by dh_resnet18_train_end.
 *   forward_train : x_dev float32[n][3][P][P] (must stay alive until backward) -> logits
 *   backward      : dlogits_dev float32[n][n_classes] -> every parameter gradient
 *   dh_ce_loss    : mean cross entropy of logits vs int64 labels -> *loss_dev, and (optional)
 *                   dlogits_dev = (softmax - onehot)/n
 *   adam_step     : one Adam update of all parameters from the current gradients (step >= 1),
 *                   then re-packs the MFMA weight copies
 *   train_tensor  : copy one tensor by state_dict name between the library and caller memory
 *                   (host or device): kind 0 parameter, 1 gradient, 2 running statistic;
 *                   to_lib != 0 writes into the library (call train_repack after parameters). */
int dh_resnet18_train_begin(dh_resnet18* net, int64_t n, int32_t patch, void* stream);
int dh_resnet18_train_end(dh_resnet18* net);
int dh_resnet18_forward_train(dh_resnet18* net, const float* x_dev, int64_t n, int32_t patch,
                              float* logits_dev, void* stream);
int dh_resnet18_backward(dh_resnet18* net, const float* dlogits_dev, void* stream);
int dh_ce_loss(const float* logits_dev, const int64_t* labels_dev, int64_t n, int32_t n_cls,
               float* loss_dev, float* dlogits_dev, void* stream);
int dh_resnet18_adam_step(dh_resnet18* net, float lr, float beta1, float beta2, float eps,
                          int64_t step, void* stream);
/* backward + Adam of a single-rank step in one call: each residual block's update and repack follow its weight
 * gradients on the engine's side stream.  Bit-identical to dh_resnet18_backward + dh_resnet18_adam_step; refused
 * while gradient buckets are armed. */
int dh_resnet18_backward_adam(dh_resnet18* net, const float* dlogits_dev, float lr, float beta1, float beta2,
                              float eps, int64_t step, void* stream);
int dh_resnet18_train_tensor(dh_resnet18* net, const char* name, int32_t kind, void* ptr,
                             int64_t n_elem, int32_t to_lib, void* stream);
int dh_resnet18_train_repack(dh_resnet18* net, void* stream);
/* Device pointer + element count of a whole arena (kind as above): data-parallel training
 * all-reduces the gradient arena in place (RCCL) between backward and adam_step. */
int dh_resnet18_train_flat(dh_resnet18* net, int32_t kind, void** ptr_out, int64_t* n_out);
/* Gradient buckets for the overlapped all-reduce of data-parallel training: the gradient arena is cut
 * into buckets of about bucket_bytes (0 = one) in the order the backward pass completes them (from the END of the arena:
 * fc, layer4 ... layer1, stem); `cb(bucket, offset, count, user)` is called on the calling thread from inside
 * dh_resnet18_backward as soon as the kernels that complete a bucket are enqueued. */
int dh_resnet18_set_buckets(dh_resnet18* net, int64_t bucket_bytes,
                            void (*cb)(int32_t bucket, int64_t offset, int64_t count, void* user), void* user,
                            int32_t* n_buckets_out);
int dh_resnet18_bucket(dh_resnet18* net, int32_t i, int64_t* offset, int64_t* count);

/* ---- configs[4]: ResNet-50 (and ResNet-18) training / evaluation in bf16 ---------------------------
 * The same step (models/patch_cls_simple/train.py:166-172; CrossEntropyLoss(mean) :117, Adam :118) for the network the
 * factory of models/patch_cls_simple/model.py:5-11 returns when it is given a ResNet-50 backbone (BASELINE.json
 * configs[4]: torchvision resnet50 v1.5 + fc[n_cls, 2048]; "resnet18" selects the reference's own backbone).
 * Activations and their gradients are bf16 (bf16 MFMA, f32 accumulation: forward, dgrad AND wgrad); master weights,
 * gradients, Adam moments and BN statistics are float32.  Parameters are set / read by torchvision state_dict name
 * with dh_train2_tensor (kind 0 parameter, 1 gradient, 2 running statistic; host or device pointers).
 *   forward(training != 0): batch-statistic BN, running statistics updated; x_dev float32[n][3][P][P] must stay alive
 *                           until backward.  forward(training == 0): BN from the running statistics (evaluation).
 *   backward              : dlogits float32[n][n_classes] -> every gradient (no float atomics: reproducible)
 *   adam_step             : step <= 0 uses the library's own step count
 *   set_buckets           : cut the gradient arena (laid out in backward-completion order, fc first) into buckets of about
 *                           bucket_bytes; `cb` is called on the calling thread inside backward as soon as the kernels that
 *                           complete a bucket are enqueued -- the hook for the bucketed, overlapped RCCL all-reduce of
 *                           data-parallel training.  dh_train2_bucket returns a bucket's element range. */
typedef struct dh_train2 dh_train2;
typedef void (*dh_bucket_cb)(int32_t bucket, int64_t offset, int64_t count, void* user);
int dh_train2_create(dh_train2** out, const char* arch, int32_t n_classes);
void dh_train2_destroy(dh_train2* net);
int dh_train2_tensor(dh_train2* net, const char* name, int32_t kind, void* ptr, int64_t n_elem, int32_t to_lib,
                     void* stream);
int dh_train2_flat(dh_train2* net, int32_t kind, void** ptr_out, int64_t* n_out);
int dh_train2_set_buckets(dh_train2* net, int64_t bucket_bytes, dh_bucket_cb cb, void* user, int32_t* n_buckets_out);
int dh_train2_bucket(dh_train2* net, int32_t i, int64_t* offset, int64_t* count);
/* optional bf16 wire format of the gradient exchange (either engine's arena; n % 4 == 0): float32 -> bf16 (round to nearest even)
 * before a bucket's all-reduce, bf16 sums -> float32 * scale (1 / world) after it.  Halves the bytes on xGMI.  A finite value past the
 * largest bf16 packs to infinity, infinities are kept, and every NaN stays a (quiet) NaN.  Refused with DH_EINVAL, dh_last_error
 * naming the argument: n not a multiple of 4, a float32 pointer not 16-byte aligned, a bf16 pointer not 8-byte aligned. */
int dh_grad_pack_bf16(const float* src_dev, uint16_t* dst_dev, int64_t n, void* stream);
int dh_grad_unpack_bf16(const uint16_t* src_dev, float* dst_dev, int64_t n, float scale, void* stream);
int dh_train2_forward(dh_train2* net, const float* x_dev, int64_t n, int32_t patch, float* logits_dev,
                      int32_t training, void* stream);
int dh_train2_backward(dh_train2* net, const float* dlogits_dev, void* stream);
int dh_train2_adam_step(dh_train2* net, float lr, float beta1, float beta2, float eps, int64_t step, void* stream);
/* backward + Adam of a single-rank step in one call: each residual block's update and bf16 repack follow its weight gradients on the
 * engine's side stream.  Bit-identical to dh_train2_backward + dh_train2_adam_step; refused while gradient buckets are armed. */
int dh_train2_backward_adam(dh_train2* net, const float* dlogits_dev, float lr, float beta1, float beta2, float eps, int64_t step,
                            void* stream);
/* ---- f1: coverage map of FullImageRndSampler (patch_samplers/full_samplers.py:63-153) ---------------------------
 * The reference keeps a float hit-count map at 1/speedup scale and, per batch, draws B tile origins from the cells hit
 * fewer than dense_level times (np.random.choice over the whole map), until every cell was hit.  The host planner
 * (deephisto_amd/coverage.py) draws every random number in the reference's order and reduces the choice to RANKS among
 * the eligible cells in row-major order; this handle owns the int32 map [dh][dw] (dh = h / speedup, dw = w / speedup)
 * and turns ranks into cells, origins and hits.  One handle per sampler; its calls are not thread-safe.
 *   create         : zeroed map; dense_level >= 1; 1 <= max_batch <= 4096 and max_batch <= dh*dw (the reference's
 *                    top-up never ends on a smaller map).  Asynchronous on `stream`.
 *   step           : one batch of n <= max_batch tiles.  idx_host: int32[n] ranks in [0, eligible) (explicit_cells = 0)
 *                    or flat cell indices in [0, dh*dw) (explicit_cells != 0: the forced top-up path);
 *                    jitter_host: int32[n][2] (jy, jx) in [0, speedup).  Origin k =
 *                    clamp((cell // dw - P//speedup//2) * speedup + jy, 0, h-P), same for x with cell % dw
 *                    (full_samplers.py:144-153); written as int32[n][2] (y, x) to origins_dev (may be NULL), then every
 *                    origin adds 1 over [y//d, (y+P)//d) x [x//d, (x+P)//d) (duplicates included; integer atomics).
 *                    Ranks / cells / jitter go up in one staged copy, the counters (and the origins when host_origins
 *                    != 0) come back in one copy; nothing is synchronised except the previous step's read-back (the
 *                    host arrays are consumed before the call returns).
 *   counters       : waits for the last step's read-back: *filled = cells hit at least once, *eligible = cells hit
 *                    fewer than dense_level times; origins_host (may be NULL; the last step must have asked for host
 *                    origins): int32[n][2] of the last step.
 *   eligible_cells : the rare top-up path: the (at most max_batch) eligible cells as sorted flat indices in
 *                    cells_host[cap], count in *n_out; synchronises `stream`.
 *   read_map       : float32[dh][dw] copy of the counts into map_dev (the reference's `_accum`).  Asynchronous.
 *   destroy        : waits for the device, frees everything (NULL is a no-op). */
typedef struct dh_coverage dh_coverage;
int dh_coverage_create(dh_coverage** out, int64_t h, int64_t w, int32_t patch, int32_t speedup, int32_t dense_level,
                       int32_t max_batch, void* stream);
int dh_coverage_step(dh_coverage* cov, const int32_t* idx_host, const int32_t* jitter_host, int32_t n, int32_t explicit_cells,
                     int32_t* origins_dev, int32_t host_origins, void* stream);
int dh_coverage_counters(dh_coverage* cov, int64_t* filled, int64_t* eligible, int32_t* origins_host);
int dh_coverage_eligible_cells(dh_coverage* cov, int32_t* cells_host, int32_t cap, int32_t* n_out, void* stream);
int dh_coverage_read_map(dh_coverage* cov, float* map_dev, void* stream);
void dh_coverage_destroy(dh_coverage* cov);

/* ---- t1: tissue mask for whole-slide prediction -------------------------------
 * Not in the reference, which classifies every tile.  A pixel is tissue when its chroma
 * max(R,G,B) - min(R,G,B) exceeds `threshold` (0..255); a tile is kept when its P x P window holds at
 * least `min_pixels` tissue pixels.  Integer work only, so the result is exact.  slide_dev:
 * uint8[h][w][3], 16-byte aligned.
 * dh_tissue_histogram: hist_dev = uint64[256] chroma histogram of the whole slide (zeroed by the call).
 * dh_tissue_tile_counts: counts_dev[i] = tissue pixels of the window at yx_dev[i] (int32[n][2], (y, x),
 *   any origin with 0 <= y <= h-P, 0 <= x <= w-P; a device origin outside the slide gets -1).  bitmap_dev is
 *   the caller's workspace of bitmap_words >= ceil(h*w / 64) uint64 words (one bit per pixel).  When
 *   yx_host_check != NULL (the same n pairs on the host) every origin is checked before any launch.
 * dh_tissue_select: kept_idx_dev = int32[k] indices i with counts_dev[i] >= min_pixels in increasing
 *   order, kept_yx_dev (optional) = their origins int32[k][2]; both need capacity n.  status_dev: int32[2]
 *   device workspace (k, origins counted -1).  With n_kept_host != NULL the call synchronises the stream,
 *   stores k, and refuses a count of -1.
 * dh_fill_uncovered: map_dev int64[h/d][w/d] cells outside the footprint [y/d, (y+P)/d) x [x/d, (x+P)/d)
 *   (clipped) of every origin of yx_dev get fill_class; cover_dev: uint8[h/d * w/d] workspace. */
int dh_tissue_histogram(const uint8_t* slide_dev, int64_t h, int64_t w, uint64_t* hist_dev, void* stream);
int dh_tissue_tile_counts(const uint8_t* slide_dev, int64_t h, int64_t w, const int32_t* yx_dev,
                          const int32_t* yx_host_check, int64_t n, int32_t patch, int32_t threshold,
                          uint64_t* bitmap_dev, int64_t bitmap_words, int32_t* counts_dev, void* stream);
int dh_tissue_select(const int32_t* counts_dev, const int32_t* yx_dev, int64_t n, int32_t min_pixels,
                     int32_t* kept_idx_dev, int32_t* kept_yx_dev, int32_t* status_dev, int64_t* n_kept_host,
                     void* stream);
int dh_fill_uncovered(const int32_t* yx_dev, int64_t n, int32_t patch, int32_t downscale, int64_t h, int64_t w,
                      int64_t fill_class, uint8_t* cover_dev, int64_t* map_dev, void* stream);

/* ---- n1: Macenko stain normalisation of the resident slide -------------------
 * No counterpart in the reference, which reads the scanner's raw RGB.  Integer work only, so the result is
 * exact: a channel's optical density is od[v], the host's 256-entry fixed-point table (12 fractional bits,
 * every value in [0, 22713]; od_dev on the device for the kernels, od_host the same values for the check
 * before any launch); a pixel is stained when max(R,G,B) <= vmax.  slide_dev: uint8[h][w][3], 16-byte
 * aligned, h*w <= dh_stain_max_pixels() (the largest slide whose 64-bit product sums cannot overflow).
 * Small fixed-point operands (eigenvectors, pseudo-inverse, matrix) are host pointers, row-major.
 * dh_stain_moments: moments_dev = uint64[10] over the stained pixels (zeroed by the call): count, the sums
 *   of od[R], od[G], od[B], then the product sums RR, RG, RB, GG, GB, BB.
 * dh_stain_angle_hist: hist_dev = uint64[n_bins] (zeroed by the call), n_bins = 1024.  p = evec_host
 *   (int32[2][3], |.| <= 2^14) . od; bounds_dev: int32[n_bins][2] directions (x, y) of the lower bin edges,
 *   counter-clockwise from angle -pi, entry 256 q the axis that opens quadrant q.  Quadrant by the signs of
 *   p, then the largest k of the quadrant with x_k * p1 - y_k * p0 >= 0.
 * dh_stain_conc_hist: hist_dev = uint64[2][n_bins] (zeroed by the call), n_bins = 2048: stain s of a
 *   stained pixel counts in bin clamp((pinv_host[s] . od) >> shift, 0, n_bins - 1); pinv_host: int32[2][3],
 *   |.| <= 2^19.
 * dh_stain_apply: every pixel, glass included: out channel c = lut_dev[clamp((matrix_host[c] . od) >> shift,
 *   0, lut_n - 1)]; matrix_host: int32[3][3], |.| <= 2^19; lut_n <= 24576.  out_dev: uint8[h][w][3], 16-byte
 *   aligned; it may be slide_dev itself (in place) and must not overlap it otherwise. */
int64_t dh_stain_max_pixels(void);
int dh_stain_moments(const uint8_t* slide_dev, int64_t h, int64_t w, const int32_t* od_dev, const int32_t* od_host,
                     int32_t vmax, uint64_t* moments_dev, void* stream);
int dh_stain_angle_hist(const uint8_t* slide_dev, int64_t h, int64_t w, const int32_t* od_dev, const int32_t* od_host,
                        int32_t vmax, const int32_t* evec_host, const int32_t* bounds_dev, int32_t n_bins,
                        uint64_t* hist_dev, void* stream);
int dh_stain_conc_hist(const uint8_t* slide_dev, int64_t h, int64_t w, const int32_t* od_dev, const int32_t* od_host,
                       int32_t vmax, const int32_t* pinv_host, int32_t shift, int32_t n_bins, uint64_t* hist_dev,
                       void* stream);
int dh_stain_apply(const uint8_t* slide_dev, int64_t h, int64_t w, const int32_t* od_dev, const int32_t* od_host,
                   const int32_t* matrix_host, int32_t shift, const uint8_t* lut_dev, int32_t lut_n, uint8_t* out_dev,
                   void* stream);

/* ---- n2: pyramid layers of the resident slide ---------------------------------
 * The reference reads layer L of a .psi file through psimage; for a slide that is an array in HBM this is the
 * layer: an integer-exact area average of src_dev = uint8[h][w][3] by the rational factor num/den >= 1,
 * 1 <= den <= num <= 2048 and num <= 64 * den (reduced by their gcd inside the call).
 *   Output size: oh = (h * den) / num, ow = (w * den) / num: only output pixels whose footprint lies wholly
 *     inside the source exist, the ragged remainder is dropped.  oh and ow are passed in and checked;
 *     oh == 0 or ow == 0 is refused.
 *   Weights: wy(y, j) = max(0, min((j+1)*den, (y+1)*num) - max(j*den, y*num)), wx the same in x; the weights of
 *     one output pixel sum to num per axis.
 *   Sum and rounding: S = sum_j sum_i wy * wx * src[j][i][c], D = num * num, out = (2*S + D) / (2*D) in
 *     integers: the exact mean rounded half up, once.
 *   Overflow: 2*S + D <= 511 * 2048^2 < 2^32.
 *   src_dev and dst_dev = uint8[oh][ow][3] are 16-byte aligned; all byte offsets are 64-bit (h, w <= 2^20);
 *     dst must not overlap src (refused before the launch). */
int dh_resample_area(const uint8_t* src_dev, int64_t h, int64_t w, int32_t num, int32_t den, uint8_t* dst_dev,
                     int64_t oh, int64_t ow, void* stream);

/* ---- n3: dihedral views of the resident slide, for test-time augmentation ------
 * A mirrored or turned tile of a slide is the plain tile, at a mapped origin, of the mirrored or turned slide;
 * this builds that slide.  view = k + 4 * f with k in 0..3 and f in 0..1:
 *     dst = np.rot90(np.fliplr(src) if f else src, k)        over axes (0, 1)
 * for src_dev = uint8[h][w][3]; the channel triple is never reordered.  dst_dev is uint8[h][w][3] for even k and
 * uint8[w][h][3] for odd k, 3 * h * w bytes either way.  View 0 is a copy.  One quarter turn sends pixel (y, x)
 * to (w - 1 - x, y), the mirror sends it to (y, w - 1 - x).
 *   Every destination byte is a source byte: no arithmetic, no float, no atomics.  All byte offsets are 64-bit;
 *     1 <= h, w <= 2^20.  Neither pointer needs any alignment.
 *   Refused with DH_EINVAL (reason in dh_last_error): a view outside 0..7, h or w below 1 (or above 2^20), a null
 *     pointer, dst == src or any overlap of the two ranges of 3 * h * w bytes. */
int dh_slide_dihedral(const uint8_t* src_dev, int64_t h, int64_t w, int32_t view, uint8_t* dst_dev, void* stream);

/* ---- q1: tile quality: out-of-focus and ink-marked tiles -----------------------
 * Not in the reference, which classifies every tile.  Integer work only, so the result is exact.  Per pixel
 * (R, G, B) of slide_dev = uint8[h][w][3] (any alignment): luma Y = (77 R + 150 G + 29 B + 128) >> 8;
 * c = max - min of the three; tissue: c > threshold (-1..255; -1: every pixel); ink: (c > ink_chroma and
 * G - min(R, B) >= ink_margin) or max(R, G, B) <= dark_max (ink_chroma, ink_margin in 0..255, dark_max in
 * -1..255; -1 switches the dark clause off).  L = 4 Y - the four neighbours' Y; a neighbour outside the slide
 * is the edge pixel (clamped coordinates), a neighbour outside the tile is the slide's pixel.
 * dh_quality_tile_stats: stats_dev = int64[n][4], per window of side patch <= 1024 at yx_dev[i] (int32[n][2],
 *   (y, x), any origin with 0 <= y <= h-P, 0 <= x <= w-P): n_t = tissue pixels, S1 = sum of L and S2 = sum of
 *   L*L over the tissue pixels, n_ink = ink pixels over all P*P.  A device origin outside the slide gets four
 *   times -1 and reads nothing.  When yx_host_check != NULL (the same n pairs on the host) every origin is
 *   checked before any launch.
 * dh_quality_flags: reason_dev[i] (uint8) = 2 (blur) when n_t*S2 - S1*S1 < min_sharpness * n_t*n_t (n_t == 0:
 *   when min_sharpness > 0), | 4 (ink) when n_ink > max_ink_pixels; keep_dev[i] (int32) = 1 when the mask is 0,
 *   else 0: dh_tissue_select(keep_dev, yx_dev, n, 1, ...) compacts the kept tiles in order.  The products stay
 *   below 2^63 for sums of tiles with patch <= 1024 and min_sharpness in [0, 1020^2], which is all the
 *   comparison is defined for.  Sums of -1 give reason 255 and keep -1, which dh_tissue_select refuses. */
int dh_quality_tile_stats(const uint8_t* slide_dev, int64_t h, int64_t w, const int32_t* yx_dev,
                          const int32_t* yx_host_check, int64_t n, int32_t patch, int32_t threshold, int32_t ink_chroma,
                          int32_t ink_margin, int32_t dark_max, int64_t* stats_dev, void* stream);
int dh_quality_flags(const int64_t* stats_dev, int64_t n, int64_t min_sharpness, int64_t max_ink_pixels,
                     uint8_t* reason_dev, int32_t* keep_dev, void* stream);

/* ---- measurement -----------------------------------------------------------------
 * Times the dominant kernel (3x3 stride-1 conv, ~85 % of the model FLOPs) with HIP
 * events recorded on the launch stream around every `sample_every`-th launch (at most
 * max_samples).  dh_profile_stop waits for the sampled launches and returns the summed
 * kernel time, the summed algorithmic FLOPs (2*pixels*cout*9*cin) and the sample count. */
int dh_profile_start(int32_t sample_every, int32_t max_samples);
int dh_profile_stop(double* total_ms, double* total_flops, int64_t* n_samples);

#ifdef __cplusplus
}
#endif
#endif /* DEEPHISTO_HIP_H */
