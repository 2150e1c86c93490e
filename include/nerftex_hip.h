/*
 * nerftex_hip.h -- C ABI of libnerftex_hip.so (MI355X / gfx950).
 *
 * This is the drop-in boundary for the instant-ngp-style rendering hot path of
 * yihua7/NeRF-Texture.  Every entry point replaces ONE function the reference's
 * pybind11 modules export (cited per function as file:line under the reference
 * checkout); the arguments keep the reference's order and meaning, with
 *   at::Tensor      ->  raw device pointer (the caller allocates everything),
 *   implicit stream ->  explicit `stream` (a hipStream_t passed as void*; NULL =
 *                       the legacy default stream the reference launches on),
 *   void / throw    ->  int status (0 = ok) + nerftex_last_error().
 *
 * Conventions
 *   - All pointers are DEVICE pointers unless the parameter is named host_*.
 *   - Every function only enqueues work on `stream`; nothing synchronises.
 *   - Outputs that the reference requires the caller to pre-zero keep that
 *     contract (flagged "pre-zeroed" below).
 *   - dtype tags: NERFTEX_F32 = 0, NERFTEX_F16 = 1 (IEEE binary16).
 *   - Error texts mirror the reference's (TORCH_CHECK / std::runtime_error
 *     messages) so a Python shim can raise RuntimeError with the same string.
 */
#ifndef NERFTEX_HIP_H
#define NERFTEX_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NERFTEX_OK 0
#define NERFTEX_ERR_INVALID 1   /* bad argument (unsupported C/D/width ...)      */
#define NERFTEX_ERR_HIP 2       /* a HIP runtime call / launch failed            */

#define NERFTEX_F32 0
#define NERFTEX_F16 1

/* layout of the per-level feature tensor handed across the boundary */
#define NERFTEX_LAYOUT_LBC 0    /* [L, B, C]  (reference native layout)          */
#define NERFTEX_LAYOUT_BLC 1    /* [B, L*C]   (what grid.py returns to callers)  */
/* OR-ed into `layout` of nerftex_grid_encode_backward(_affine): grad_embeddings arrives UNINITIALISED and is overwritten (the
 * reference's contract, and the default here, is a zero-filled buffer the kernels add into -- gridencoder/grid.py:74).  Saves
 * the caller's fill pass over the table; the large-batch path then writes every row itself.                               */
#define NERFTEX_LAYOUT_GRAD_OVERWRITE 0x100

/* opaque handle of a triangle mesh + its BVH on the device (the RayTracer section below) */
typedef struct nerftex_raytracer nerftex_raytracer;

/* Test aid: bit mask of the library scratch slots (march 0, compaction 1, MLP 2 / 8, hash grid 3 / 4 / 5, occupancy 6 / 7) that calls have
 * asked for since this function was last called.  Two replayed graphs may run concurrently only if their masks are disjoint
 * (INTEGRATION.md "Scratch memory and streams"). [extension] */
unsigned nerftex_workspace_slots_touched(void);

/* Stream captures record against ONE library scratch set by default, so two graphs that use the same slot must not be replayed side by side
 * (INTEGRATION.md "Scratch memory and streams").  A caller that WANTS to replay such graphs concurrently -- the ray ranges of an inference
 * frame, each a chain of compaction / march / field / compositing launches on its own stream -- records each of them under its own set:
 * captures made by the calling thread after nerftex_workspace_capture_set(k) use set k (0 = the default; 0 .. 255), until it is changed
 * back.  Graphs recorded under different sets share no scratch. [extension, round 5] */
int nerftex_workspace_capture_set(int set);

/* "Rows per unit" arguments of the device-count entry points (n_step of nerftex_march_rays_dev / nerftex_composite_rays_dev, rows_per_unit of
 * nerftex_grid_encode_forward_rows / nerftex_field_forward_rows) may be this code instead of a number: every kernel of the iteration then derives
 * n_step = clamp(F * N / alive, F, 8 F) -- the rule of nerf/renderer.py:470 with F N sample slots per iteration -- from the alive count on the
 * device, so that a whole iteration can be recorded into a HIP graph without the host knowing the count.  N < 2^24 rays, F <= 127; buffers
 * sized for F * N (+ 128) rows. [extension, round 5] */
#define NERFTEX_ROWS_AUTO(N, F) (0x80000000u | ((uint32_t)(F) << 24) | (uint32_t)(N))

/* Debugging aid: where the library's scratch of `slot` for `stream` (NULL = the default stream) currently sits and how large it is (*ptr = NULL,
 * *bytes = 0 if none has been allocated).  Nothing is allocated.  The contents are whatever the last call that used the slot left -- for slot 5
 * (hash-grid backward) the directory, the partial tiles and the record regions, in that order (csrc/gridencoder_binned.hip). [extension] */
int nerftex_debug_workspace(int slot, void* stream, void** ptr, size_t* bytes);

/* thread-local text of the last error on this thread ("" if none) */
const char* nerftex_last_error(void);
/* library / build identification: "nerftex_hip <ver> gfx950" */
const char* nerftex_version(void);

/* Tuning knobs / A-B switches of the kernels (profiling aid; the defaults are what is measured and shipped).  The library
 * reads its environment ONCE when it is loaded (NERFTEX_TUNE="name=value,..."), a launch never calls getenv().  Names:
 * grid_fwd, grid_bwd, grid_bwd_sweep, grid_bwd_items, grid_bwd_slice, grid_bwd_nomerge, grid_bwd_probe,
 * march, march_serial, ffmlp_wg_per_cu, ffmlp_bwd_split, march_lean, grid_bwd_stage, composite_keep,
 * march_count_probe (the one list in csrc/common.hpp documents the values).
 * tune_set: NERFTEX_ERR_INVALID for an unknown name; tune_get: -1 for an unknown name.                                    */
int nerftex_tune_set(const char* name, long value);
long nerftex_tune_get(const char* name);

/* The library's scratch (INTEGRATION.md "Scratch memory and streams": one grow-only buffer per device, stream and purpose -- the march's
 * accepted-t log alone is N * max_steps floats, capped at 1 GiB) is kept for the life of the process.  After a one-off oversized call
 * (a force_all_rays march of a whole image, say) this frees all of it, on every device; the next calls allocate again at their own size.
 * Synchronises the devices first.  NOT while a captured graph that uses the library may still be replayed: its kernels hold the addresses. */
int nerftex_release_workspaces(void);

/* Optional per-kernel device timing (hipEvent pairs recorded on the launch stream around every kernel the
 * library launches).  on = 0 off (default), 1 every kernel, 2 hash-grid kernels only; bench.py uses 2 over its timed
 * region to report the roofline kernel's average launch duration.  report() synchronises the device and writes a JSON object
 * {"kernel": {"calls": n, "avg_us": x, "total_us": y}, ...} into buf (truncated to n bytes, NUL-terminated).      */
int nerftex_profile_enable(int on);
int nerftex_profile_reset(void);
int nerftex_profile_report(char* buf, size_t n);

/* ------------------------------------------------------------------------- *
 * gridencoder  (reference: gridencoder/src/bindings.cpp:5-8,
 *               gridencoder/src/gridencoder.h:12-13, gridencoder.cu:419-474)
 * ------------------------------------------------------------------------- */

/* replaces _gridencoder.grid_encode_forward (gridencoder.cu:419-442).
 *   inputs      [B, D]   float32 in [0,1]
 *   embeddings  [rows,C] dtype
 *   offsets     [L+1]    int32
 *   outputs     layout LBC: [L,B,C] | BLC: [B,L*C]   dtype
 *   dy_dx       [B, L*D*C] dtype (only touched when calc_grad_inputs)
 *   S = log2(per_level_scale), H = base resolution, gridtype 0=hash 1=tiled
 * errors: "GridEncoding: C must be 1, 2, 4, or 8." for bad C and bad D (sic). */
int nerftex_grid_encode_forward(const float* inputs, const void* embeddings, const int32_t* offsets,
                                void* outputs, uint32_t B, uint32_t D, uint32_t C, uint32_t L,
                                float S, uint32_t H, int calc_grad_inputs, void* dy_dx,
                                uint32_t gridtype, int align_corners, int dtype, int layout,
                                void* stream);

/* replaces _gridencoder.grid_encode_backward (gridencoder.cu:444-474).
 *   grad            LBC: [L,B,C] | BLC: [B,L*C]   dtype
 *   grad_embeddings [rows,C] dtype, pre-zeroed, accumulated with atomics
 *   grad_inputs     [B,D] dtype (written iff calc_grad_inputs; uses dy_dx)      */
int nerftex_grid_encode_backward(const void* grad, const float* inputs, const void* embeddings,
                                 const int32_t* offsets, void* grad_embeddings, uint32_t B,
                                 uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H,
                                 int calc_grad_inputs, const void* dy_dx, void* grad_inputs,
                                 uint32_t gridtype, int align_corners, int dtype, int layout,
                                 void* stream);

/* Install the host copy of a level table (offsets_host [L+1]) for the device table at offsets_dev.  The large-batch backward
 * plans its launch from a host copy.  A table it has not been told about is learnt WITHOUT blocking: an asynchronous copy into
 * pinned memory is started on the call's stream and the launches that arrive before it has landed run the path that needs no
 * host copy (slower, same results); under stream capture an unknown table is NERFTEX_ERR_INVALID.  A caller that may pass a NEW
 * table at a recycled address must register it: the kernels compare the device table with the host copy, and on a mismatch the
 * launch writes NO gradient and raises a deferred error (below) -- nothing traps, nothing synchronises.  The Python wrapper
 * registers every offsets tensor it sees for the first time.  [extension: the reference reads offsets on the device only]   */
int nerftex_grid_register_offsets(const int32_t* offsets_dev, uint32_t L, const int32_t* offsets_host);

/* Deferred (asynchronous) error of an earlier launch, reported once: NERFTEX_ERR_INVALID + nerftex_last_error() text if a
 * hash-grid backward launch found its device offsets table different from the registered host copy, else NERFTEX_OK.  Meaningful
 * after the stream has been synchronised; the next nerftex_grid_encode_backward* call reports (and clears) it as well.
 * [extension]                                                                                                             */
int nerftex_deferred_error(void);

/* The hash table's clustering regulariser (gridencoder/grid_clustering.py:93-217, tools/map.py:747-774 of the reference): per level
 * l, rows x = table[offsets[l] : offsets[l+1]] against centres[l] [K, C],
 *   q = normalise_rows((1 + |x - c|^2 / alpha)^(-(alpha + 1) / 2)),  p = normalise_rows(q^2 / colsum(q)) (detached),
 *   loss = weight * sum over the levels of mean_{i,k} p (log p - log q)   (KLDivLoss(reduction='mean')).
 * *level (device int32): 0..L-1 = that level, -1 = every level summed (the reference's pick_level=False); anything else writes a
 * NaN loss and no gradient.  grad_table / grad_centres (optional): grad_scale * d loss / d x is ADDED into the level's rows of
 * grad_table [rows, C], grad_scale * d loss / d centres into grad_centres [L, K, C]; grad_scale is a device float (NULL = 1).
 * Nothing is read back, allocated or synchronised: capturable.  No float atomics: the same bits on every run.  C in {1, 2, 4, 8},
 * 1 <= K <= 16, alpha > 0; max_level_rows (host) is the largest level's row count -- it sizes the launch, the kernels take each
 * level's count from offsets.  scratch: caller-owned, 16-byte aligned, nerftex_grid_cluster_scratch_bytes(desc) bytes (it depends
 * on C, K, L and max_level_rows only).  [extension: the reference evaluates the loss with ~30 framework ops on the host's level pick] */
typedef struct nerftex_grid_cluster_desc {
    const float* table;      /* [offsets[L], C] fp32 */
    const int32_t* offsets;  /* device [L + 1] */
    uint32_t C, L, K;
    uint32_t max_level_rows;
    const float* centres;    /* [L, K, C] fp32 */
    float alpha;
    float weight;
    const int32_t* level;    /* device int32 */
    const float* grad_scale; /* device, may be NULL */
    float* loss;             /* device fp32 scalar, written */
    float* grad_table;       /* may be NULL */
    float* grad_centres;     /* may be NULL */
    void* scratch;
    size_t scratch_bytes;
} nerftex_grid_cluster_desc;
int nerftex_grid_cluster_scratch_bytes(const nerftex_grid_cluster_desc* desc, size_t* bytes);
int nerftex_grid_cluster_loss(const nerftex_grid_cluster_desc* desc, void* stream);

/* The same two calls with the caller's coordinate normalisation folded in: every kernel reads x = (inputs + in_add) * in_mul
 * (two fp32 roundings, as the framework's add and multiply before the call: gridencoder/grid.py:141 with in_add = bound,
 * in_mul = 1 / (2 bound)).  dy_dx / grad_inputs stay derivatives with respect to the NORMALISED x; in_mul > 0.             */
int nerftex_grid_encode_forward_affine(const float* inputs, const void* embeddings, const int32_t* offsets, void* outputs,
                                       uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H,
                                       int calc_grad_inputs, void* dy_dx, uint32_t gridtype, int align_corners, int dtype,
                                       int layout, float in_add, float in_mul, void* stream);
int nerftex_grid_encode_backward_affine(const void* grad, const float* inputs, const void* embeddings,
                                        const int32_t* offsets, void* grad_embeddings, uint32_t B, uint32_t D, uint32_t C,
                                        uint32_t L, float S, uint32_t H, int calc_grad_inputs, const void* dy_dx,
                                        void* grad_inputs, uint32_t gridtype, int align_corners, int dtype, int layout,
                                        float in_add, float in_mul, void* stream);

/* ------------------------------------------------------------------------- *
 * shencoder  (reference: shencoder/src/bindings.cpp, shencoder.h:10,13,
 *             shencoder.cu:386-440).  float32 only (the wrapper forces it,
 *             shencoder/sphere_harmonics.py:16).
 * ------------------------------------------------------------------------- */

/* replaces _shencoder.sh_encode_forward.  inputs [B,3], outputs [B,C*C],
 * dy_dx [B,3,C*C] (iff calc_grad_inputs).  C = degree in 1..8.               */
int nerftex_sh_encode_forward(const float* inputs, float* outputs, uint32_t B, uint32_t D,
                              uint32_t C, int calc_grad_inputs, float* dy_dx, void* stream);

/* replaces _shencoder.sh_encode_backward.  grad [B,C*C]; grad_inputs [B,3]
 * pre-zeroed, accumulated into (+=) exactly like shencoder.cu:359-383.       */
int nerftex_sh_encode_backward(const float* grad, const float* inputs, uint32_t B, uint32_t D,
                               uint32_t C, const float* dy_dx, float* grad_inputs, void* stream);

/* ------------------------------------------------------------------------- *
 * raymarching  (reference: raymarching/src/bindings.cpp:5-21,
 *               raymarching.h:7-19).  All float tensors are float32 (every
 *               wrapper uses custom_fwd(cast_inputs=float32)).
 * ------------------------------------------------------------------------- */

/* raymarching.cu:150-158.  aabb [6]; miss -> near = far = FLT_MAX.           */
int nerftex_near_far_from_aabb(const float* rays_o, const float* rays_d, const float* aabb,
                               uint32_t N, float min_near, float* nears, float* fars,
                               void* stream);
/* raymarching.cu:203-211.  coords [N,2] in [-1,1].                           */
int nerftex_polar_from_ray(const float* rays_o, const float* rays_d, float radius, uint32_t N,
                           float* coords, void* stream);
/* raymarching.cu:231-234 / 259-262.  10 bits per axis.                       */
int nerftex_morton3D(const int32_t* coords, uint32_t N, int32_t* indices, void* stream);
int nerftex_morton3D_invert(const int32_t* indices, uint32_t N, int32_t* coords, void* stream);
/* raymarching.cu:294-302.  N = number of output BYTES; bit i of byte n is
 * grid[8n+i] > density_thresh.                                               */
int nerftex_packbits(const float* grid, uint32_t N, float density_thresh, uint8_t* bitfield,
                     void* stream);

/* raymarching.cu:485-494 (kernel :314-483).
 *   grid     density bitfield [C*H^3/8] uint8
 *   xyzs/dirs [M,3], deltas [M,2]  pre-zeroed
 *   rays     [N,3] int32 (ray id, point offset, num_steps)
 *   counter  [2] int32, ACCUMULATED into: counter[0] += total points,
 *            counter[1] += N  (same end state as the reference's atomics)
 *   perturb  0/1; the RNG is pcg32 seeded 42, advanced by the ray id.
 * Unlike the reference (two global atomics per ray, arbitrary order) the ray
 * records are emitted in ray order with prefix-sum offsets: deterministic.
 * H must be a power of two (the Morton index of any other grid runs past
 * C*H^3 bits, in the reference as well).  Dispatch, the same bits on every
 * path (tests/test_gpu_march_paths.py):
 *   H <= 256  the data-parallel count pass + the expanding pass (knob
 *             march_lean = 1: the count pass compiled for fewer registers;
 *             march_serial = 1: the serial count pass, as for H > 256);
 *   H > 256   the serial count pass (one ray per lane, logging the accepted
 *             parameters) + the expanding pass: the data-parallel pass packs
 *             voxel coordinates into 8 bits each;
 *   replay    knob march = 1, or a log N * max_steps * 4 bytes above 1 GiB:
 *             the serial count pass without a log, then a second serial walk
 *             per ray that writes the samples.                               */
int nerftex_march_rays_train(const float* rays_o, const float* rays_d, const uint8_t* grid,
                             float bound, float dt_gamma, uint32_t max_steps, uint32_t N,
                             uint32_t C, uint32_t H, uint32_t M, const float* nears,
                             const float* fars, float* xyzs, float* dirs, float* deltas,
                             int32_t* rays, int32_t* counter, uint32_t perturb, void* stream);
/* EXTENSION (no reference counterpart): the training march as the trainer calls
 * it every step -- near_far_from_aabb (raymarching.py:22-51), counter.zero_()
 * (nerf/renderer.py:366-368), three zero-filled sample buffers
 * (raymarching.py:184-186), march_rays_train -- as ONE call of two launches:
 * near / far are computed inside the counting pass (same arithmetic) and STORED
 * to nears / fars [N]; the counter is taken as zero and overwritten
 * (counter[0] = total points, counter[1] = N); xyzs | dirs | deltas may arrive
 * uninitialised (they must be consecutive parts of ONE buffer of 8 M floats):
 * the rows no ray writes are zeroed by the second launch.  Same samples, ray
 * records and counter as the four-step sequence, bit for bit.
 * H a power of two; the two-launch form is that of the data-parallel count
 * pass (H <= 256, march_serial and march unset, and a log N * max_steps * 4
 * bytes of at most 1 GiB).  On the serial and replay paths, chosen by a knob,
 * by H > 256 or by a log above 1 GiB (see nerftex_march_rays_train), the call
 * makes the steps it stands for
 * -- a near / far launch and ONE fill of the 8 M floats and the counter --
 * and then the plain march: four launches, the same bits.                    */
int nerftex_march_rays_train_fresh(const float* rays_o, const float* rays_d, const uint8_t* grid,
                                   float bound, float dt_gamma, uint32_t max_steps, uint32_t N,
                                   uint32_t C, uint32_t H, uint32_t M, const float* aabb,
                                   float min_near, float* nears, float* fars, float* xyzs,
                                   float* dirs, float* deltas, int32_t* rays, int32_t* counter,
                                   uint32_t perturb, void* stream);
/* raymarching.cu:671-678 (kernel :506-669): as nerftex_march_rays_train
 * (H a power of two, the same dispatch by H and by the knobs, the same bits
 * on every path) + rays_ts [M] = t after each emitted step.                  */
int nerftex_march_rays_train_differentiable(const float* rays_o, const float* rays_d,
                                            const uint8_t* grid, float bound, float dt_gamma,
                                            uint32_t max_steps, uint32_t N, uint32_t C, uint32_t H,
                                            uint32_t M, const float* nears, const float* fars,
                                            float* xyzs, float* dirs, float* deltas,
                                            float* rays_ts, int32_t* rays, int32_t* counter,
                                            uint32_t perturb, void* stream);
/* raymarching.cu:780-788 (kernel :700-777).                                  */
int nerftex_composite_rays_train_forward(const float* sigmas, const float* rgbs,
                                         const float* deltas, const int32_t* rays, uint32_t M,
                                         uint32_t N, float* weights_sum, float* depth,
                                         float* image, void* stream);
/* raymarching.cu:884-892 (kernel :802-881). grad_sigmas/grad_rgbs pre-zeroed. */
int nerftex_composite_rays_train_backward(const float* grad_weights_sum, const float* grad_image,
                                          const float* sigmas, const float* rgbs,
                                          const float* deltas, const int32_t* rays,
                                          const float* weights_sum, const float* image, uint32_t M,
                                          uint32_t N, float* grad_sigmas, float* grad_rgbs,
                                          void* stream);
/* raymarching.cu:1009-1017 (kernel :900-1006).  xyzs/dirs/deltas pre-zeroed;
 * perturb doubles as the pcg32 seed.                                         */
int nerftex_march_rays(uint32_t n_alive, uint32_t n_step, const int32_t* rays_alive,
                       const float* rays_t, const float* rays_o, const float* rays_d, float bound,
                       float dt_gamma, uint32_t max_steps, uint32_t C, uint32_t H,
                       const uint8_t* grid, const float* nears, const float* fars, float* xyzs,
                       float* dirs, float* deltas, uint32_t perturb, void* stream);
/* raymarching.cu:1097-1104 (kernel :1021-1094).  In-place accumulate.        */
int nerftex_composite_rays(uint32_t n_alive, uint32_t n_step, const int32_t* rays_alive,
                           float* rays_t, const float* sigmas, const float* rgbs,
                           const float* deltas, float* weights_sum, float* depth, float* image,
                           void* stream);
/* raymarching.cu:1136-1142 (kernel :1117-1134).  alive_counter[0] += number
 * kept.  Order-preserving (ballot + prefix sum) instead of atomics order.    */
int nerftex_compact_rays(uint32_t n_alive, int32_t* rays_alive, const int32_t* rays_alive_old,
                         float* rays_t, const float* rays_t_old, int32_t* alive_counter,
                         void* stream);

/* ------------------------------------------------------------------------- *
 * Extension: everything of the ngp field behind the hash-grid
 * gather as ONE kernel -- nerf/network_ff.py:85-101: sigma net (32 -> 64 -> 64 -> 16,
 * ReLU), trunc_exp of output 0, SH degree 4 of the view direction, colour net
 * ([SH | geometry features | 0] -> 64 -> 64 -> 64 -> 16), sigmoid of outputs 0..2.
 *   feats_lbc [16, B, 2] half: the LEVEL-MAJOR features (layout NERFTEX_LAYOUT_LBC of
 *   nerftex_grid_encode_forward: what the XCD-pinned gather kernel writes; no transpose);
 *   dirs [B, 3] fp32; sigma_weights / color_weights: the two FFMLP weight vectors (half);
 *   sigma [B] fp32, rgbs [B, 3] fp32 (half-valued, as the unfused sequence gives them).
 * Training additionally gets what the backward entry points read (all three or none; hc, the colour net's raw outputs, is
 * optional on top -- nothing downstream needs it):
 *   x_rows [B, 32] (the features as rows), h [B, 16], cin [B, 32], hc [B, 16] or NULL, half.
 * B % 128 == 0.  Same values, bit for bit, as grid rows -> nerftex_ffmlp_forward ->
 * nerftex_field_mid_forward -> nerftex_ffmlp_forward -> nerftex_field_out_forward.
 * ------------------------------------------------------------------------- */
int nerftex_field_forward(const void* feats_lbc, const float* dirs, const void* sigma_weights, const void* color_weights,
                          uint32_t B, float* sigma, float* rgbs, void* x_rows, void* h, void* cin, void* hc, void* stream);

/* ------------------------------------------------------------------------- *
 * Extension (backward): the backward of the ngp field behind the gather in
 * THREE launches -- the two recomputing MLP backward kernels with the field's glue folded into
 * their load stage (the colour net's output gradient is formed from grad_rgbs and rgbs:
 * nerftex_field_out_backward; the sigma net's from grad_sigma, h and the colour net's input
 * gradient: nerftex_field_mid_backward) and ONE reduction of both networks' weight-gradient
 * partials -- for nerftex_field_out_backward + nerftex_ffmlp_backward + nerftex_field_mid_backward
 * + nerftex_ffmlp_backward (six launches); no grad_hc / grad_h tensors.
 *   in:  grad_sigma [B] fp32, grad_rgbs [B,3] fp32, rgbs [B,3] fp32 (as nerftex_field_forward
 *        returned them), h [B,16], cin [B,32], x_rows [B,32] half (its training side outputs),
 *        the two weight vectors;
 *   out: grad_cin [B,32] half (the colour net's input gradient: scratch for the caller),
 *        grad_x [B,32] half (dL/dfeatures, rows -> nerftex_grid_encode_backward),
 *        grad_sigma_weights, grad_color_weights (half, overwritten).
 * Bit-identical gradients.  B % 128 == 0; fp16 only.
 * ------------------------------------------------------------------------- */
int nerftex_field_backward(const float* grad_sigma, const float* grad_rgbs, const float* rgbs, const void* h, const void* cin,
                           const void* x_rows, const void* sigma_weights, const void* color_weights, uint32_t B, void* grad_cin,
                           void* grad_x, void* grad_sigma_weights, void* grad_color_weights, void* stream);

/* Extension (round 4): GradScaler's non-finite scan (torch/amp/grad_scaler.py `_unscale_grads_` -> found_inf; the reference trainer's
 * scaler.step, nerf/utils.py:1005-1009) done by the kernels that WRITE the gradients instead of by a pass that re-reads them:
 * the same calls as nerftex_field_backward / nerftex_grid_encode_backward_affine, and *found_inf (a device float) is set to 1.0f when an
 * element of grad_sigma_weights / grad_color_weights, resp. of grad_embeddings, comes out inf or nan.  Never cleared here (the
 * optimizer step clears it: nerftex_adam_half_step_amp); found_inf NULL = the plain call.  Paths of the hash-grid backward whose
 * stores cannot carry the test (small batches: atomics) scan the finished table in one more launch -- the contract holds for all.
 * Two limits a C caller must know (the Python harness satisfies both):
 *   - the scan covers the values THIS call writes.  With NERFTEX_LAYOUT_GRAD_OVERWRITE every row is written by the call, so it covers the
 *     whole table; in ACCUMULATE mode (the reference's pre-zeroed buffer, the default layout) rows whose contribution from this call is
 *     zero are not rewritten and an inf / nan ALREADY in grad_embeddings there is not seen -- scan an accumulated gradient with
 *     nerftex_amp_check_half instead;
 *   - *found_inf is sticky until an optimizer step (nerftex_adam_half_step_amp) or nerftex_amp_update clears it: a caller that DISCARDS a
 *     backward pass without stepping must zero it itself, or the next, unrelated step is skipped.                                      */
int nerftex_field_backward_amp(const float* grad_sigma, const float* grad_rgbs, const float* rgbs, const void* h, const void* cin,
                               const void* x_rows, const void* sigma_weights, const void* color_weights, uint32_t B, void* grad_cin,
                               void* grad_x, void* grad_sigma_weights, void* grad_color_weights, float* found_inf, void* stream);
int nerftex_grid_encode_backward_amp(const void* grad, const float* inputs, const void* embeddings, const int32_t* offsets,
                                     void* grad_embeddings, uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H,
                                     int calc_grad_inputs, const void* dy_dx, void* grad_inputs, uint32_t gridtype, int align_corners,
                                     int dtype, int layout, float in_add, float in_mul, float* found_inf, void* stream);

/* Extension (round 5): the fused ngp field with its two networks in bf16 (BASELINE configs[2] names bf16; the reference's ffmlp is fp16-only,
 * ffmlp/src/utils.h:23).  Same arguments as nerftex_field_forward / nerftex_field_backward_amp with these types: feats_lbc stays fp16 (the hash
 * table is fp16 under any autocast) and is narrowed to bf16 on load; weights, x_rows, h, cin, hc, grad_cin and the two weight gradients are
 * bf16; grad_x -- the hash-grid backward's input -- is fp16 (each element rounded to bf16 first: what autograd's cast back through the
 * unfused chain's `.to(bfloat16)` produces); sigma, rgbs, grad_sigma, grad_rgbs fp32.  found_inf may be NULL.                            */
int nerftex_field_forward_bf16(const void* feats_lbc, const float* dirs, const void* sigma_weights, const void* color_weights,
                               uint32_t B, float* sigma, float* rgbs, void* x_rows, void* h, void* cin, void* hc, void* stream);
int nerftex_field_backward_bf16(const float* grad_sigma, const float* grad_rgbs, const float* rgbs, const void* h, const void* cin,
                                const void* x_rows, const void* sigma_weights, const void* color_weights, uint32_t B, void* grad_cin,
                                void* grad_x, void* grad_sigma_weights, void* grad_color_weights, float* found_inf, void* stream);
/* Extension (round 6): nerftex_field_backward_amp / _bf16 over the 32-row steps the compositing backward flagged as carrying a gradient
 * (step_live[B / 32], 0 = all 32 rows have exactly zero grad_sigma and grad_rgbs: nerftex_composite_tail_backward_live).  A dead step adds exact
 * zeros to the weight gradients and has a zero input gradient (ffmlp/src/ffmlp.cu:410-518 computes those zeros): it issues no loads and no MFMAs;
 * its rows of grad_x are written as zeros (two stores per lane: the hash-grid backward reads every row), its rows of grad_cin -- which only the
 * second kernel of this call reads, on live steps -- are NOT WRITTEN.  The step -> wave assignment is that of the plain call, so every gradient
 * is the plain call's, bit for bit.  found_inf may be NULL.                                                                               */
int nerftex_field_backward_live(const float* grad_sigma, const float* grad_rgbs, const float* rgbs, const void* h, const void* cin,
                                const void* x_rows, const void* sigma_weights, const void* color_weights, uint32_t B, void* grad_cin,
                                void* grad_x, void* grad_sigma_weights, void* grad_color_weights, const uint32_t* step_live, float* found_inf,
                                void* stream);
int nerftex_field_backward_live_bf16(const float* grad_sigma, const float* grad_rgbs, const float* rgbs, const void* h, const void* cin,
                                     const void* x_rows, const void* sigma_weights, const void* color_weights, uint32_t B, void* grad_cin,
                                     void* grad_x, void* grad_sigma_weights, void* grad_color_weights, const uint32_t* step_live, float* found_inf,
                                     void* stream);
/* ... and the same as the LAST stage of a step's loss side: CONSUMING the flags -- when the call's launches have run, step_live[0 .. B / 32) is zero
 * again (the weight-gradient reduction clears what the two backward kernels have walked) -- and, with `loss`, finishing the step's loss: one extra
 * workgroup of that reduction launch adds the rays' squared errors nerftex_composite_step left in err[] (called with loss = NULL) in
 * nerftex_render_tail_forward's order -- off the step's critical path, where a launch of its own costs 5 us.  The counterpart of
 * nerftex_composite_step, which sets flags and has no launch before it to clear them.  step_live NULL: the plain backward; loss NULL: none.        */
typedef struct nerftex_step_loss {
    const float* err;    /* [n_rays] squared error per ray (nerftex_composite_step) */
    uint32_t n_rays;     /* 1 .. 262144 */
    float loss_mul;
    const float* scale;  /* device float or NULL */
    float* loss;         /* [1] out: mean squared error * loss_mul */
    float* scaled_loss;  /* [1] out or NULL: loss * *scale */
} nerftex_step_loss;
int nerftex_field_backward_live_consume(const float* grad_sigma, const float* grad_rgbs, const float* rgbs, const void* h, const void* cin,
                                        const void* x_rows, const void* sigma_weights, const void* color_weights, uint32_t B, void* grad_cin,
                                        void* grad_x, void* grad_sigma_weights, void* grad_color_weights, uint32_t* step_live,
                                        const nerftex_step_loss* loss, float* found_inf, void* stream);
int nerftex_field_backward_live_consume_bf16(const float* grad_sigma, const float* grad_rgbs, const float* rgbs, const void* h, const void* cin,
                                             const void* x_rows, const void* sigma_weights, const void* color_weights, uint32_t B, void* grad_cin,
                                             void* grad_x, void* grad_sigma_weights, void* grad_color_weights, uint32_t* step_live,
                                             const nerftex_step_loss* loss, float* found_inf, void* stream);
/* ... and nerftex_field_backward_live_consume WITHOUT its reduction launch (round 6): `_deferred` runs the two backward kernels and DESCRIBES the rest --
 * the weight-gradient reduction (+ found_inf), the flags' clearing, the step's loss -- in *trailer (opaque; the partial sums wait in the library's
 * scratch: no other nerftex_ffmlp_* / nerftex_field_* backward call in between).  nerftex_grid_encode_backward_adam_trailer, the step's next long
 * launch, runs the trailer on the first workgroups of its fill kernel: nothing before the optimizer reads what the trailer writes, and as a launch of
 * its own it sat 8 us on the step's critical path.  nerftex_step_trailer_run runs it as that launch of its own (what the caller does when the
 * hash-grid call returned an error -- it has launched nothing then).  Same sums in the same order either way.                                  */
typedef struct nerftex_step_trailer { uint64_t opaque[16]; } nerftex_step_trailer;
int nerftex_field_backward_live_deferred(const float* grad_sigma, const float* grad_rgbs, const float* rgbs, const void* h, const void* cin,
                                         const void* x_rows, const void* sigma_weights, const void* color_weights, uint32_t B, void* grad_cin,
                                         void* grad_x, void* grad_sigma_weights, void* grad_color_weights, uint32_t* step_live,
                                         const nerftex_step_loss* loss, float* found_inf, nerftex_step_trailer* trailer, void* stream);
int nerftex_field_backward_live_deferred_bf16(const float* grad_sigma, const float* grad_rgbs, const float* rgbs, const void* h, const void* cin,
                                              const void* x_rows, const void* sigma_weights, const void* color_weights, uint32_t B, void* grad_cin,
                                              void* grad_x, void* grad_sigma_weights, void* grad_color_weights, uint32_t* step_live,
                                              const nerftex_step_loss* loss, float* found_inf, nerftex_step_trailer* trailer, void* stream);
int nerftex_step_trailer_run(const nerftex_step_trailer* trailer, void* stream);
/* ... and the two no-grad forms of the bf16 field: the density query of the occupancy-grid update (nerftex_field_density) and the inference
 * iteration sized by a device count (nerftex_field_forward_rows, declared below), weights bf16, feats_lbc fp16, outputs fp32.  Same values as
 * nerftex_field_forward_bf16's sigma / (sigma, rgbs) on the rows they compute. */
int nerftex_field_density_bf16(const void* feats_lbc, const void* sigma_weights, uint32_t B, float* sigma, void* stream);
int nerftex_field_forward_rows_bf16(const void* feats_lbc, const float* dirs, const void* sigma_weights, const void* color_weights,
                                    uint32_t B, float* sigma, float* rgbs, const int32_t* units_dev, uint32_t rows_per_unit,
                                    void* stream);

/* Extension (round 4): the table gradient in PARTS, for a data-parallel caller that exchanges it level group by level group: the
 * all-reduce of the rows of levels [lo, hi) can start as soon as those levels are summed, while the later levels are still being summed
 * (replaces the single gradient exchange after the backward pass; the reference only has the dormant DDP wrap, nerf/utils.py:439-441).
 *   phase 1: bin the contributions of EVERY level (the first kernel of the large-batch backward); grad_embeddings is not written;
 *   phase 2: sum (and combine) the tiles of levels [level_lo, level_hi): rows offsets[lo] .. offsets[hi] of grad_embeddings are final;
 *   phase 3: both.  Same arguments as nerftex_grid_encode_backward_affine without the input gradient.
 * The phase-2 calls read the scratch the phase-1 call left: same stream (or everything inside stream captures), same B, no other
 * hash-grid backward of this library in between.  Large-batch path only (C = 2, B >= 16384, a registered level table): anything
 * else is NERFTEX_ERR_INVALID -- the caller falls back to the one-call backward.  Same bits as the one-call backward. */
int nerftex_grid_encode_backward_phase(const void* grad, const float* inputs, const void* embeddings, const int32_t* offsets,
                                       void* grad_embeddings, uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H,
                                       uint32_t gridtype, int align_corners, int dtype, int layout, float in_add, float in_mul, int phase,
                                       uint32_t level_lo, uint32_t level_hi, void* stream);

/* Extension (round 6): the hash-grid table backward that ALSO applies the optimizer's update.  (The reference leaves the optimizer to torch:
 * main_nerf.py:128 `torch.optim.Adam(betas=(0.9, 0.99), eps=1e-15)` under the GradScaler of nerf/utils.py:1003-1009; this is
 * nerftex_grid_encode_backward_amp + nerftex_adam_mixed_step_amp on the table, fused where the gradient is still on chip.)
 * The tiles of the hashed levels have one owner each in the summing kernel; that owner rounds the tile's exact row sums to fp16 -- the values
 * grad_embeddings would have held -- and applies Adam to the rows itself: grad_embeddings receives ONLY rows [0, *first_updated_row) (the coarse
 * levels whose tiles several work items share; host word, written before the call returns, a function of the level table and B), every row
 * from there on is updated and gets NO gradient written.
 * GradScaler skips a WHOLE step when any gradient element of any tensor is non-finite, which no tile can know about the tiles behind it, so the
 * optimizer state is DOUBLE-BUFFERED: the call reads set [*live & 1] of param / exp_avg / exp_avg_sq and writes the other set; *found_inf is
 * raised when a row's gradient comes out inf / nan (it is not read here).  The caller ends the step with nerftex_adam_mixed_step_amp_db, which
 * updates what is left (rows [0, first_updated_row) and its other tensors) the same way, flips *live iff the step is applied and, on a skipped
 * step, re-derives the fp16 copy this call rewrote in place (param_half) from the live fp32 set.
 * fp16 tables, C = 2, NERFTEX_LAYOUT_GRAD_OVERWRITE, a registered level table whose levels are multiples of 4 rows; everything else is refused. */
/* Extension: a learning-rate schedule on the device -- torch.optim.lr_scheduler.LambdaLR as the reference trains with it (main_nerf.py:131-133:
 * lr = base_lr * 0.1 ** min(iter / iters, 1), stepped after every optimizer step, skipped ones included, nerf/utils.py:1020-1025).  Training step
 * number t (*iter) uses base_lr * factor[min(t, n - 1)], the product in double as LambdaLR forms it in Python; the launch that ends a step (the
 * loss scaler's tail of the _sched Adam entries, or nerftex_lr_schedule_publish) advances *iter by one, whether the step is applied or skipped.
 * A replayed graph reads the step's rate from here instead of holding the rate of its capture.  factor: device double [n], n >= 1; iter: device
 * word.  The descriptor itself is a host struct, read when the call is made.                                                               */
typedef struct nerftex_lr_schedule {
    const double* factor;
    uint32_t n;
    uint32_t* iter;
} nerftex_lr_schedule;

typedef struct nerftex_table_adam {
    float* param[2];       /* fp32 table, state sets 0 and 1, [rows, 2] each */
    float* exp_avg[2];
    float* exp_avg_sq[2];
    void* param_half;      /* the fp16 table the forward reads: rewritten in place for the updated rows */
    const uint32_t* live;  /* device word: which set holds the current state */
    const float* step;     /* device: completed optimizer steps (this update is number *step + 1) */
    const float* grad_scale; /* device, may be NULL: gradients are divided by it */
    float* found_inf;      /* device: raised on inf / nan */
    double lr, beta1, beta2, eps;
    const nerftex_lr_schedule* sched; /* may be NULL: train at lr.  Else lr is the base rate and the step's rate is read from the schedule, before
                                         the step's last launch advances it (the counter this step will end with)                              */
} nerftex_table_adam;
int nerftex_grid_encode_backward_adam(const void* grad, const float* inputs, const int32_t* offsets, void* grad_embeddings, uint32_t B,
                                      uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H, uint32_t gridtype, int align_corners, int dtype,
                                      int layout, float in_add, float in_mul, const nerftex_table_adam* adam, uint32_t* first_updated_row,
                                      void* stream);
/* ... with the step's trailer (nerftex_field_backward_live_deferred, above) run by the first workgroups of the fill launch.  An error return has
 * launched nothing.                                                                                                                              */
int nerftex_grid_encode_backward_adam_trailer(const void* grad, const float* inputs, const int32_t* offsets, void* grad_embeddings, uint32_t B,
                                              uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H, uint32_t gridtype, int align_corners,
                                              int dtype, int layout, float in_add, float in_mul, const nerftex_table_adam* adam,
                                              uint32_t* first_updated_row, const nerftex_step_trailer* trailer, void* stream);

/* Extension (round 4): the density query of the field alone -- nerf/network_ff.py:103-117 `density`: hash-grid features -> sigma net ->
 * trunc_exp -- for the occupancy-grid update (nerf/renderer.py:566-660 queries 2-4 M cell positions every 16 steps).
 *   feats_lbc [16, B, 2] half (nerftex_grid_encode_forward*, NERFTEX_LAYOUT_LBC), sigma_weights as nerftex_field_forward's,
 *   sigma [B] float out.  Same values as nerftex_field_forward's sigma.  B % 128 == 0; fp16 weights (bf16: nerftex_field_density_bf16). */
int nerftex_field_density(const void* feats_lbc, const void* sigma_weights, uint32_t B, float* sigma, void* stream);


/* ------------------------------------------------------------------------- *
 * Extension (the sync-free inference loop): the two field launches of
 * an inference iteration sized by an UPPER BOUND of the alive-ray count -- the loop of
 * nerf/renderer.py:455-483 without its `alive_counter.item()` -- skip the rows that carry
 * nothing: only the first units_dev[0] * rows_per_unit points (alive rays x n_step) are
 * encoded / shaded, the rest of the outputs is left untouched (nerftex_composite_rays_dev
 * never reads it).  Otherwise nerftex_grid_encode_forward_affine (no dy_dx) and the
 * inference form of nerftex_field_forward; units_dev NULL = all B rows.
 * ------------------------------------------------------------------------- */
int nerftex_grid_encode_forward_rows(const float* inputs, const void* embeddings, const int32_t* offsets, void* outputs,
                                     uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H, uint32_t gridtype,
                                     int align_corners, int dtype, int layout, float in_add, float in_mul,
                                     const int32_t* units_dev, uint32_t rows_per_unit, void* stream);
int nerftex_field_forward_rows(const void* feats_lbc, const float* dirs, const void* sigma_weights, const void* color_weights,
                               uint32_t B, float* sigma, float* rgbs, const int32_t* units_dev, uint32_t rows_per_unit,
                               void* stream);

/* ------------------------------------------------------------------------- *
 * Extension: the curved-field projector in one kernel --
 * MeshProjector.project (tools/map.py:414-433) with its coarse normal from the K
 * nearest mesh vertices (knn(), :454-501, use_dir_vec=True, Shepard weights), the
 * two closest-hit traces along +-normal, the nearer hit as surface point / signed
 * height / face id / tangent frame, the height mask, and FreqEncoder(height)
 * (tools/encoding.py:5-43, tools/map.py:635).  The neighbour search itself (frnn,
 * un-vendored) stays with the caller: knn_idx / knn_dist are its output.
 *   xyz [N,3]; knn_idx [N,K] int32 (a negative index counts from the end, as the framework's vertex_normals[idx] does with frnn's
 *   -1 padding; anything else outside [0, n_verts) is clamped into it); knn_dist [N,K] (euclidean, ascending);
 *   mesh_vertices, vertex_normals [n_verts,3]; tbn [F,9] or NULL; n_freqs = multires;
 *   p_sur [N,3]; sdf [N]; h_mask [N] uint8; normal [N,3]; face_idx [N] int64
 *   (-1: no hit within 10); tbn_out [N,9] or NULL; z_embed [N, 1 + 2 n_freqs] or NULL.
 * ------------------------------------------------------------------------- */
int nerftex_curved_project(const nerftex_raytracer* rt, const float* xyz, const int32_t* knn_idx, const float* knn_dist,
                           uint32_t N, uint32_t K, const float* mesh_vertices, const float* vertex_normals, uint32_t n_verts,
                           float dir_vec_wdist, float h_threshold, const float* tbn, uint32_t n_freqs, float* p_sur,
                           float* sdf, uint8_t* h_mask, float* normal, int64_t* face_idx, float* tbn_out,
                           float* z_embed, void* stream);

/* ------------------------------------------------------------------------- *
 * Extension: the neighbour search of the curved-field projector --
 * the role of frnn.frnn_grid_points (un-vendored FRNN) at tools/map.py:396 (grid over the
 * mesh vertices, built once) and :456 (K nearest vertices per sample point, sorted, with a
 * radius that never binds).  EXACT K nearest: a uniform grid built on the host from
 * host_points [V,3], searched ring by ring on the device until the K-th best distance
 * cannot be beaten by an unvisited cell.
 *   idx [N,K] int32 ascending by distance (equal distances inside one cell: by index),
 *   dist [N,K] EUCLIDEAN distances (what MeshProjector.knn() computes with dis.sqrt()).
 * 1 <= K <= min(16, V).
 * ------------------------------------------------------------------------- */
typedef struct nerftex_knn nerftex_knn;
int nerftex_knn_create(const float* host_points, uint32_t n_points, nerftex_knn** out);
int nerftex_knn_destroy(nerftex_knn* knn);
int nerftex_knn_query(const nerftex_knn* knn, const float* xyz, uint32_t N, uint32_t K, int32_t* idx, float* dist, void* stream);

/* ------------------------------------------------------------------------- *
 * Extension: the inference loop without a host stall.
 * nerf/renderer.py:455-470 reads the number of alive rays back every iteration
 * (`alive_counter.item()`) to size the next launches; here the launches are sized
 * by an upper bound the host already has (the count of the PREVIOUS iteration:
 * alive rays never increase) and the kernels read the true count from the device.
 * Same arithmetic per ray as the three reference-shaped entry points above.
 * nerftex_march_rays_dev does NOT need zero-filled outputs (the reference-shaped
 * nerftex_march_rays does, raymarching.py:385-387): it writes dt = 0, a position far
 * outside the box (1e30: the grid encoder returns zeros for it without a gather) and
 * 1e30 as the direction's first component (nerftex_field_forward_rows skips a
 * wave-step whose 32 rows are all marked like that) into the slots a ray leaves
 * unused -- compositing stops at the first dt == 0, raymarching.cu:1076; the rest of
 * those slots keeps whatever the buffer held and reaches no output.
 * ------------------------------------------------------------------------- */
int nerftex_march_rays_dev(uint32_t n_alive_bound, const int32_t* n_alive_dev, uint32_t n_step, const int32_t* rays_alive,
                           const float* rays_t, const float* rays_o, const float* rays_d, float bound, float dt_gamma,
                           uint32_t max_steps, uint32_t C, uint32_t H, const uint8_t* grid, const float* fars, float* xyzs,
                           float* dirs, float* deltas, uint32_t perturb, void* stream);
int nerftex_composite_rays_dev(uint32_t n_alive_bound, const int32_t* n_alive_dev, uint32_t n_step, const int32_t* rays_alive,
                               float* rays_t, const float* sigmas, const float* rgbs, const float* deltas, float* weights_sum,
                               float* depth, float* image, void* stream);
/* n_alive_dev[0]: alive entries of the old arrays; alive_counter[0] is overwritten with the number of survivors (a different word). */
int nerftex_compact_rays_dev(uint32_t n_alive_bound, const int32_t* n_alive_dev, int32_t* rays_alive, const int32_t* rays_alive_old,
                             float* rays_t, const float* rays_t_old, int32_t* alive_counter, void* stream);
/* Extension (round 6): nerftex_compact_rays_dev + the loop condition of nerf/renderer.py:459-483 (`while step < max_steps: ... step += n_step`) kept
 * ON THE DEVICE, for a loop whose iterations are recorded HIP graphs: steps_done[0] (zero when the frame starts) is the sum of the n_step of the
 * iterations so far; an iteration that finds it >= max_steps reports 0 survivors -- every later kernel of the recorded iterations then does
 * nothing -- otherwise it adds this iteration's n_step (a plain number, or NERFTEX_ROWS_AUTO(N, F): derived from the survivors, as the
 * iteration's other kernels derive it).                                                                                              */
int nerftex_compact_rays_budget_dev(uint32_t n_alive_bound, const int32_t* n_alive_dev, int32_t* rays_alive, const int32_t* rays_alive_old,
                                    float* rays_t, const float* rays_t_old, int32_t* alive_counter, uint32_t* steps_done, uint32_t max_steps,
                                    uint32_t n_step, void* stream);
/* Extension (round 6): the same, and the kernel also writes the survivor count to host_mirror[0] -- pinned host memory that the device can address
 * (hipHostMalloc, torch's pin_memory) -- so that a host loop which wants to know how many rays are left needs no copy node behind the launch (such a
 * 4-byte copy is a kernel of its own: 9-41 us median, 110-170 us at the 95th percentile when other streams keep the CUs busy).  Read host_mirror[0]
 * after an event recorded behind this launch has completed; if later launches on the same word have run by then it holds THEIR count -- in
 * nerf/renderer.py:459-483's loop, whose alive count only falls, still an upper bound of what is left.  host_mirror == NULL is an error.      */
int nerftex_compact_rays_budget_mirror_dev(uint32_t n_alive_bound, const int32_t* n_alive_dev, int32_t* rays_alive, const int32_t* rays_alive_old,
                                           float* rays_t, const float* rays_t_old, int32_t* alive_counter, uint32_t* steps_done, uint32_t max_steps,
                                           uint32_t n_step, int32_t* host_mirror, void* stream);

/* ------------------------------------------------------------------------- *
 * Extension: occupancy-grid maintenance on the device --
 * NeRFRenderer.update_extra_state (nerf/renderer.py:566-660) without its
 * framework glue, torch.nonzero and .item() read-backs.  Given the same random
 * numbers (noise / rand_coords / rand_pick, each optional: NULL = the library's
 * counter-based generator keyed by `seed`) the grid and bitfield equal what the
 * reference's Python computes.
 * Accepted shapes, all four entry points: 1 <= cascade <= 8; H a power of two,
 * 8 ... 1024 (cells are indexed by their 3-D Morton code, which runs past H^3
 * for any other grid size); cascade * H^3 < 2^32 and cascade * rows per
 * cascade (2 N, rows_per_cascade) < 2^32 (cell and row indices are 32-bit).
 * Anything else returns NERFTEX_ERR_INVALID before any allocation or launch
 * (tests/test_gpu_occupancy_edges.py holds the kernels against a host model
 * at H = 8 ... 64).
 * ------------------------------------------------------------------------- */

/* Full sweep (renderer.py:579-605): jittered query position of every cell of every cascade, row = cas * H^3 + Morton index,
 * so that the density estimates of these rows ARE the Morton-ordered grid.  xyzs [cascade*H^3, 3]; noise [cascade*H^3, 3] in [0,1). */
int nerftex_occupancy_sample_full(float* xyzs, uint32_t cascade, uint32_t H, float bound, const float* noise,
                                  uint64_t seed, void* stream);

/* Partial update (renderer.py:609-637): per cascade N uniformly random cells (rows 0..N-1 of the cascade's 2N) and N cells drawn from
 * the currently occupied ones (density_grid > 0, ascending order like torch.nonzero; rows N..2N-1, index -1 when there is none).
 *   density_grid [cascade, H^3]; rand_coords [cascade, N, 3] int32 in [0,H); rand_pick [cascade, N] int32 in [0, occupied count);
 *   noise [cascade*2N, 3]; indices [cascade, 2N] int32 (Morton cell index); xyzs [cascade*2N, 3];
 *   n_occupied [cascade] uint32 (optional): the per-cascade occupied counts, left on the device.                              */
int nerftex_occupancy_sample_partial(const float* density_grid, uint32_t cascade, uint32_t H, float bound, uint32_t N,
                                     const int32_t* rand_coords, const int32_t* rand_pick, const float* noise, uint64_t seed,
                                     int32_t* indices, float* xyzs, uint32_t* n_occupied, void* stream);

/* Extension (round 5): the same with the draws STRATIFIED when `stratified` != 0 and no explicit rand_coords / rand_pick are given: row j of the
 * uniform half draws one of the j-th run of H^3 / N consecutive Morton indices (N must divide H^3), row j of the occupied half one entry of the
 * j-th of N equal slices of the occupied list -- every cell still has the probability N / H^3 of being named (the reference's N iid draws
 * with replacement, renderer.py:611, name ~0.885 N distinct cells; these name N), and the rows come out in ASCENDING Morton order, so the
 * density query over them has the full sweep's locality in the hash table instead of none (0.81 -> 0.6 ms per update on an MI355X).      */
int nerftex_occupancy_sample_partial_ordered(const float* density_grid, uint32_t cascade, uint32_t H, float bound, uint32_t N,
                                             const int32_t* rand_coords, const int32_t* rand_pick, const float* noise, uint64_t seed,
                                             int32_t* indices, float* xyzs, uint32_t* n_occupied, int stratified, void* stream);

/* renderer.py:639-654: tmp grid from (indices, sigmas) -- indices NULL = a full sweep, sigmas [cascade, H^3] in Morton order; a cell named
 * several times takes the largest estimate --, density_grid = max(density_grid * decay, tmp) where both are >= 0 (everywhere with
 * force_full_grid), mean_thresh[0] = mean(clamp(density_grid, 0)), mean_thresh[1] = min(mean, density_thresh), bitfield = packbits at that
 * threshold.  mean_thresh: 2 floats on the device; nothing is read back.                                                       */
int nerftex_occupancy_update(float* density_grid, const float* sigmas, const int32_t* indices, uint32_t rows_per_cascade,
                             uint32_t cascade, uint32_t H, float decay, int force_full_grid, float density_thresh,
                             float* mean_thresh, uint8_t* bitfield, void* stream);

/* ------------------------------------------------------------------------- *
 * ffmlp  (reference: ffmlp/src/bindings.cpp:5-10, ffmlp.h:8-13,
 *         ffmlp.cu:630-895).  fp16 storage; MFMA with fp32 accumulation.
 *   weights  flat: [hidden,in] + (num_layers-1)*[hidden,hidden] + [out16,hidden],
 *            each row-major [out,in]  (ffmlp.cu:632)
 *   inputs [B,in] half, outputs [B,output_dim] half (output_dim = 16, padded)
 *   forward_buffer / backward_buffer [num_layers, B, hidden] half
 *   activation ids: 0 relu 1 exponential 2 sine 3 sigmoid 4 squareplus
 *                   5 softplus 6 none  (ffmlp/ffmlp.py:89-96)
 *   B must be a multiple of 128 (the Python module pads, ffmlp.py:157-159).
 * ------------------------------------------------------------------------- */
int nerftex_ffmlp_forward(const void* inputs, const void* weights, uint32_t B, uint32_t input_dim,
                          uint32_t output_dim, uint32_t hidden_dim, uint32_t num_layers,
                          uint32_t activation, uint32_t output_activation, void* forward_buffer,
                          void* outputs, void* stream);
int nerftex_ffmlp_inference(const void* inputs, const void* weights, uint32_t B,
                            uint32_t input_dim, uint32_t output_dim, uint32_t hidden_dim,
                            uint32_t num_layers, uint32_t activation, uint32_t output_activation,
                            void* inference_buffer, void* outputs, void* stream);
/* grad [B,output_dim] half; grad_weights flat half (every element is overwritten);
 * grad_inputs [B,in] half (written iff calc_grad_inputs); backward_buffer
 * [num_layers,B,hidden] scratch: written only by the split dgrad/wgrad path, the
 * fused kernel (hidden 64, 2..4 layers, input <= 64) leaves it untouched and
 * accepts NULL.  forward_buffer == NULL (fused kernel only): the activations
 * are rebuilt from `inputs` with the forward kernel's chain, bit-identical, so
 * a training forward may be run with nerftex_ffmlp_inference.                  */
int nerftex_ffmlp_backward(const void* grad, const void* inputs, const void* weights,
                           const void* forward_buffer, uint32_t B, uint32_t input_dim,
                           uint32_t output_dim, uint32_t hidden_dim, uint32_t num_layers,
                           uint32_t activation, uint32_t output_activation, int calc_grad_inputs,
                           void* backward_buffer, void* grad_inputs, void* grad_weights,
                           void* stream);
/* Extension: the same three entry points on bfloat16 tensors (inputs, weights, buffers, outputs, gradients all bf16; fp32 accumulation
 * on v_mfma_f32_16x16x32_bf16).  The reference has no bf16 mode (utils.h:23 accepts at::Half only); BASELINE.json configs[2] names it. */
int nerftex_ffmlp_forward_bf16(const void* inputs, const void* weights, uint32_t B, uint32_t input_dim,
                               uint32_t output_dim, uint32_t hidden_dim, uint32_t num_layers,
                               uint32_t activation, uint32_t output_activation, void* forward_buffer,
                               void* outputs, void* stream);
int nerftex_ffmlp_inference_bf16(const void* inputs, const void* weights, uint32_t B,
                                 uint32_t input_dim, uint32_t output_dim, uint32_t hidden_dim,
                                 uint32_t num_layers, uint32_t activation, uint32_t output_activation,
                                 void* inference_buffer, void* outputs, void* stream);
int nerftex_ffmlp_backward_bf16(const void* grad, const void* inputs, const void* weights,
                                const void* forward_buffer, uint32_t B, uint32_t input_dim,
                                uint32_t output_dim, uint32_t hidden_dim, uint32_t num_layers,
                                uint32_t activation, uint32_t output_activation, int calc_grad_inputs,
                                void* backward_buffer, void* grad_inputs, void* grad_weights, void* stream);

/* ffmlp.cu:711-740: the reference creates side streams for its split-K wgrad
 * GEMMs.  Here wgrad is reduced inside one launch, so these only size / drop
 * the fp32 partial-sum workspace; kept so `FFMLP.__init__` binds unchanged.  */
int nerftex_ffmlp_allocate_splitk(size_t size);
int nerftex_ffmlp_free_splitk(void);

/* ------------------------------------------------------------------------- *
 * RayTracer / BVH  (reference: external/RayTracer/src/bindings.cpp:13-18,
 *                   src/raytracer.cu:21-64, src/bvh.cu:527-721)
 * ------------------------------------------------------------------------- */

/* replaces _raytracing.create_raytracer: HOST arrays in, BVH-4 built on the
 * host (median split on the max-variance axis, <= 8 triangles per leaf),
 * nodes + reordered triangles uploaded.  *out owns the device memory.        */
int nerftex_create_raytracer(const float* host_vertices, uint32_t n_vertices,
                             const uint32_t* host_triangles, uint32_t n_triangles,
                             nerftex_raytracer** out);
int nerftex_destroy_raytracer(nerftex_raytracer* rt);
/* replaces RayTracer.trace (raytracer.cu:45-58): closest hit per ray.
 * positions/normals [N,3] (may alias rays_o/rays_d), depth [N] (10.0 on miss),
 * face_idx [N] int64 pre-filled with -1 by the caller (left untouched on miss) */
int nerftex_raytracer_trace(const nerftex_raytracer* rt, const float* rays_o, const float* rays_d,
                            float* positions, float* normals, float* depth, int64_t* face_idx,
                            uint32_t N, void* stream);

/* ------------------------------------------------------------------------- *
 * field glue  (no counterpart among the reference's native exports: these four
 *              fuse the framework-level ops nerf/network_ff.py:60-110 runs
 *              between and after the two FFMLPs -- SURVEY 8(f) N1, first step)
 * ------------------------------------------------------------------------- */

/* h [B,16] fp16 (sigma-net outputs), dirs [B,3] fp32  ->  sigma [B] fp32 = exp(h[:,0]) (trunc_exp forward,
 * tools/activation.py:9-12), cin [B,32] fp16 = [SH degree 4 of dir | h[:,1:16] | 0] (network_ff.py:88-96).     */
int nerftex_field_mid_forward(const void* h, const float* dirs, uint32_t B, float* sigma, void* cin, void* stream);
/* grad_h [B,16] fp16: column 0 = grad_sigma * exp(clamp(h0,-15,15)) (activation.py:14-17), 1..15 = grad_cin[:,16:31] */
int nerftex_field_mid_backward(const float* grad_sigma, const void* grad_cin, const void* h, uint32_t B, void* grad_h,
                               void* stream);
/* hc [B,16] fp16 (colour-net outputs) -> rgbs [B,3] fp32 = sigmoid(hc[:,:3]) rounded through fp16 (network_ff.py:99-100) */
int nerftex_field_out_forward(const void* hc, uint32_t B, float* rgbs, void* stream);
/* Extension (round 6): the same kind of glue for the CURVED field (network_curvedfield.py:283-306 around tools/map.py:620-641's MeshFeatureField):
 *   nerftex_curved_pack_inputs   x_embed [B,16] half, z_embed [B,25] fp32 -> [B,48] half = [x_embed | half(z_embed) | 1 x 7] (the sigma net's padded input)
 *   nerftex_curved_mid_forward   h [B,16] half, normal [B,3] fp32, dirs [B,3] fp32 -> sigma [B] half = exp(h[:,0]) (trunc_exp),
 *                                cin [B,32] half = [SH4 of the view direction reflected about the normal | h[:,1:16] | 1]; eval bit 0: the
 *                                fc_weight blend + renormalisation of :289-291; bit 1: `normal` is the projector's raw normal and is normalised
 *                                first as MeshFeatureField does (tools/map.py:720)
 *   nerftex_curved_out_forward   hc rows of row_stride halfs, sigma_raw [B] half, mask [B] bytes -> sigma = mask ? sigma_raw : 0,
 *                                color [B,3] half = mask ? sigmoid(hc[:, :3]) : 0
 * Forward only: their backward passes are slices / the sigmoid derivative (nerftex_field_mid_backward serves the middle one).               */
int nerftex_curved_pack_inputs(const void* x_embed, const float* z_embed, uint32_t B, void* out, void* stream);
int nerftex_curved_mid_forward(const void* h, const float* normal, const float* dirs, uint32_t B, float fc_weight, int eval, void* sigma, void* cin,
                               void* stream);
int nerftex_curved_out_forward(const void* hc, uint32_t row_stride, const void* sigma_raw, const uint8_t* mask, uint32_t B, void* sigma, void* color,
                               void* stream);
/* -------------------------------------------------------------------------
 * Extension: the curved field's whole no-grad forward as ONE call in the device-count form of nerftex_grid_encode_forward_rows /
 * nerftex_field_forward_rows, so that a renderer's inference iteration over a CurvedField can sit in a recorded HIP graph:
 *   neighbour search -> projector (writes FreqEncoder(height) as 16-bit values straight into the sigma net's input) -> hash-grid gather ->
 *   sigma net 48 -> 32 -> 16 -> trunc_exp / reflected view direction / SH -> colour net 32 -> 64 -> 64 -> 3 -> sigmoid + height mask,
 * eight launches enqueued on `stream`; nothing is allocated, the host never waits, the call can be captured.
 *   live = min(B, units_dev[0] * rows_per_unit)  (rows_per_unit a plain number or NERFTEX_ROWS_AUTO(N, F); units_dev NULL: live = B),
 *   read by every kernel of the chain from the same device word.
 *   rows >= live                      no work; sigma / rgbs keep what they held.
 *   live rows the march marked unused (dirs[row][0] > 1e29, nerftex_march_rays_dev): no search, no traversal, no table read;
 *                                     sigma = 0, rgbs = 0.
 *   every other live row              bit for bit what nerftex_knn_query, nerftex_curved_project, nerftex_grid_encode_forward_affine,
 *                                     nerftex_curved_pack_inputs, nerftex_ffmlp_inference, nerftex_curved_mid_forward, nerftex_ffmlp_inference
 *                                     and nerftex_curved_out_forward give one after the other, widened to fp32.
 * NERFTEX_ERR_INVALID with a message, before anything is launched: a NULL descriptor or a NULL handle / buffer, B % 128 != 0, K outside
 * 1..16 (or above the number of mesh vertices), n_verts outside 1..2^31-1, anything but the default curved field's shapes (n_freqs 12; table 3-D, 2 features x 8 levels,
 * fp16; sigma net 48 / 32 / 2 layers / 16; colour net 32 / 64 / 3 layers / 3), scratch smaller than nerftex_curved_field_infer_scratch_bytes(B).
 * B == 0: NERFTEX_OK, nothing launched.
 * ------------------------------------------------------------------------- */
typedef struct nerftex_curved_infer_desc {
    const nerftex_knn* knn;            /* the mesh vertices' neighbour grid (nerftex_knn_create)                                  */
    const nerftex_raytracer* tracer;   /* the mesh's BVH (nerftex_create_raytracer)                                               */
    const float* xyz;                  /* [B,3] sample positions                                                                  */
    const float* dirs;                 /* [B,3] view directions; dirs[row][0] > 1e29 marks an unused slot                         */
    uint32_t B;
    uint32_t n_verts;
    const float* mesh_vertices;        /* [n_verts,3]                                                                             */
    const float* vertex_normals;       /* [n_verts,3]                                                                             */
    const float* tbn;                  /* [F,9] per-face frames: carried for the fine-normal net, not read by the static light model */
    uint32_t K;                        /* neighbours per point                                                                    */
    uint32_t n_freqs;                  /* FreqEncoder(height) bands (multires)                                                    */
    float dir_vec_wdist;               /* weight distance of the mean direction among the normal candidates (tools/map.py:473-481) */
    float h_threshold;                 /* |height| below min(9.5, h_threshold) sets the mask                                      */
    const void* table;                 /* fp16 hash table [rows, C]                                                               */
    const int32_t* offsets;            /* [L + 1] level offsets (device)                                                          */
    uint32_t D, C, L;                  /* the gather's constants, as nerftex_grid_encode_forward_rows takes them                  */
    float S;
    uint32_t H;
    uint32_t gridtype;
    int align_corners;
    float in_add, in_mul;              /* the gather reads (p_sur + in_add) * in_mul                                              */
    const void* sigma_weights;         /* fp16, 16-byte aligned                                                                   */
    uint32_t sigma_in, sigma_hidden, sigma_layers, sigma_out;
    const void* color_weights;         /* fp16, 16-byte aligned                                                                   */
    uint32_t color_in, color_hidden, color_layers, color_out;
    float fc_weight;
    int eval;                          /* the eval bits of nerftex_curved_mid_forward                                             */
    float* sigma;                      /* [B] fp32                                                                                */
    float* rgbs;                       /* [B,3] fp32                                                                              */
    const int32_t* units_dev;
    uint32_t rows_per_unit;
    void* scratch;                     /* caller-owned, 256-byte aligned, >= nerftex_curved_field_infer_scratch_bytes(B) bytes    */
    size_t scratch_bytes;
} nerftex_curved_infer_desc;
size_t nerftex_curved_field_infer_scratch_bytes(uint32_t B);
int nerftex_curved_field_infer(const nerftex_curved_infer_desc* d, void* stream);

/* -------------------------------------------------------------------------
 * Extension: an IMPORTED planar feature texture under the curved field -- the `imported_type == 'field'` branch of MeshFeatureField.forward
 * (tools/map.py:646-668): where the mesh chain searches neighbours, traces twice and gathers a hash table, an O(1) bilinear read of a
 * [map_h, map_w, 16] fp32 image (channel-last, in the axis order MeshFeatureField.import_field receives) on the xy plane.  Per sample x, all
 * fp32, every operation rounded on its own:
 *   mode NERFTEX_PLANAR_MULTIPLY (the reference's `rescale`):  u = x0 * plane_scale0,  v = x1 * plane_scale1
 *   mode NERFTEX_PLANAR_DIVIDE:                                u = x0 / plane_scale0,  v = x1 / plane_scale1   (true divisions)
 *   sdf  = (x2 * height_scale0) * height_scale1 - sdf_offset
 *   mask = |sdf| < h_threshold (strict; no 9.5 cap here) and -1 <= u <= 1 and -1 <= v <= 1 (inclusive)
 *   features = grid_sample(bilinear, align_corners, zero padding) at (u, v), u along the map's FIRST axis: iu = ((u + 1) / 2) (map_h - 1),
 *              iv likewise, i0 = floor(iu), j0 = floor(iv); the weights (i0+1-iu)(j0+1-iv), (iu-i0)(j0+1-iv), (i0+1-iu)(iv-j0), (iu-i0)(iv-j0)
 *              on the texels (i0,j0), (i0+1,j0), (i0,j0+1), (i0+1,j0+1), four products added in that order; a corner outside the map adds nothing
 *              and is not read.  Evaluated for every row, whatever its mask (as the reference does).
 *   xin [B,48] fp16 = [half(features) | half(FreqEncoder(sdf)), 25 values: the projector's ladder | 1 x 7]   (the sigma net's padded input)
 * nerftex_planar_lookup is the plain form: any B, every row; p_uv [B,2] = (u, v), sdf [B], mask [B] bytes, xin.  NERFTEX_ERR_INVALID before
 * anything is launched, in this order: n_freqs other than 12; map_h or map_w outside 1..16384; (B == 0 returns NERFTEX_OK here;) a NULL
 * pointer, a map or xin that is not 16-byte aligned; a mode other than the two; a scale or h_threshold that is not positive and finite, an
 * sdf_offset that is not finite.
 *
 * nerftex_curved_import_infer: the whole no-grad forward over such a map as ONE call under the rows contract of nerftex_curved_field_infer --
 *   lookup -> sigma net 48 -> 32 -> 16 -> trunc_exp / reflected view direction / SH -> colour net 32 -> 64 -> 64 -> 3 -> sigmoid + mask,
 * five launches (the last four are nerftex_curved_field_infer's own), nothing allocated, capturable.  The coarse normal is (0, 0, 1), which
 * the mid kernel normalises as MeshFeatureField does (eval bit 1).
 *   rows >= live                      no work; sigma / rgbs keep what they held.
 *   live rows the march marked unused no texel read; sigma = 0, rgbs = 0.
 *   every other live row              bit for bit what nerftex_planar_lookup, nerftex_ffmlp_inference, nerftex_curved_mid_forward,
 *                                     nerftex_ffmlp_inference and nerftex_curved_out_forward give one after the other, widened to fp32.
 * NERFTEX_ERR_INVALID with a message, before anything is launched, in this order: a NULL descriptor; B % 128 != 0; n_features other than 16,
 * n_freqs other than 12 or other network shapes than sigma net 48 / 32 / 2 / 16, colour net 32 / 64 / 3 / 3; map_h or map_w outside
 * 1..16384; (B == 0 returns NERFTEX_OK here;) a NULL pointer, a scratch that is not 256-byte aligned or smaller than
 * nerftex_curved_import_infer_scratch_bytes(B); a map or weight vector that is not 16-byte aligned; a mode other than the two; a scale or
 * h_threshold that is not positive and finite, an sdf_offset that is not finite.
 * ------------------------------------------------------------------------- */
#define NERFTEX_PLANAR_MULTIPLY 0
#define NERFTEX_PLANAR_DIVIDE 1
int nerftex_planar_lookup(const float* xyz, const float* map, uint32_t map_h, uint32_t map_w, uint32_t mode, float plane_scale0, float plane_scale1,
                          float height_scale0, float height_scale1, float sdf_offset, float h_threshold, uint32_t n_freqs, uint32_t B, float* p_uv,
                          float* sdf, uint8_t* mask, void* xin, void* stream);
typedef struct nerftex_curved_import_infer_desc {
    const float* xyz;                  /* [B,3] sample positions                                                                  */
    const float* dirs;                 /* [B,3] view directions; dirs[row][0] > 1e29 marks an unused slot                         */
    uint32_t B;
    const float* map;                  /* [map_h, map_w, n_features] fp32, 16-byte aligned                                        */
    uint32_t map_h, map_w, n_features;
    uint32_t mode;                     /* NERFTEX_PLANAR_MULTIPLY / NERFTEX_PLANAR_DIVIDE                                          */
    float plane_scale0, plane_scale1;
    float height_scale0, height_scale1;
    float sdf_offset;
    float h_threshold;
    uint32_t n_freqs;                  /* FreqEncoder(height) bands (multires)                                                    */
    const void* sigma_weights;         /* fp16, 16-byte aligned                                                                   */
    uint32_t sigma_in, sigma_hidden, sigma_layers, sigma_out;
    const void* color_weights;         /* fp16, 16-byte aligned                                                                   */
    uint32_t color_in, color_hidden, color_layers, color_out;
    float fc_weight;
    int eval;                          /* the eval bits of nerftex_curved_mid_forward                                             */
    float* sigma;                      /* [B] fp32                                                                                */
    float* rgbs;                       /* [B,3] fp32                                                                              */
    const int32_t* units_dev;
    uint32_t rows_per_unit;
    void* scratch;                     /* caller-owned, 256-byte aligned, >= nerftex_curved_import_infer_scratch_bytes(B) bytes   */
    size_t scratch_bytes;
} nerftex_curved_import_infer_desc;
size_t nerftex_curved_import_infer_scratch_bytes(uint32_t B);
int nerftex_curved_import_infer(const nerftex_curved_import_infer_desc* d, void* stream);

/* -------------------------------------------------------------------------
 * Extension: the imported map on a NEW UV-MAPPED MESH -- the `imported_type == 'shape'` branch of MeshFeatureField.forward (tools/map.py:693-700)
 * over MeshProjector.uvh / barycentric_mapping (:503-543) and knn(use_dir_vec=False, weighting='DualD', nn_consis_check=True) (:454-501).  One
 * launch behind the neighbour search (nerftex_knn_query over the new mesh's vertices).  Per sample x, all fp32, every operation rounded on its
 * own (no fused multiply-add but the tracer's own o + t d):
 *   dir_k  = (x - v_k) / (|x - v_k| + 1e-5);  dis_k = dir_k . dir_0 > 0 ? knn_dist_k : 1e5;  dk = max dis, d1 = min dis
 *   w_k    = (dk - dis_k) / (dk - d1 + 1e-5) * (dk + d1) / (dk + dis_k),  w_k /= sum w  (no epsilon)
 *   normal = n / (|n| + 1e-5),  n = sum_k w_k n_k / (|n_k| + 1e-5)          knn_idx: -1 is the last vertex, anything else is clamped
 *   d1, d2 = the closest hits along +normal and -normal (10 on a miss); inner = d1 < d2; the nearer hit's face (-1 when both miss) and point
 *   sdf    = (inner ? -d1 : d2) / sdf_scale - sdf_offset                     (a true division; the caller clamps sdf_scale to >= 1e-5)
 *   mask   = |sdf| < min(9.5, h_threshold) and face != -1
 *   b      = (|p1 x p2|, |p2 x p0|, |p0 x p1|) / (their sum + 1e-5),  p_k = corner_k - p_sur        (face -1 reads face 0)
 *   (u, v) = (sum_k b_k face_uv[face][k]) * uv_rate
 *   features = nerftex_planar_lookup's bilinear read of the map at (u, v) (no box test in the mask; a corner outside the map adds nothing)
 *   xin [N,48] fp16 = [half(features) | half(FreqEncoder(sdf)) | 1 x 7]
 * A row whose normal is not finite (every kept distance ties, K == 1, x on its nearest vertex: the reference's 0 / 0) reads no face, UV or
 * texel: mask = 0, normal = 0, p_uv = 0, sdf = 0, face = -1, features 0, ladder 0 | ones.
 * nerftex_shape_lookup is the plain form: any N, every row.  face_uv [n_faces,6]: the three corners' (u, v) per face.  NERFTEX_ERR_INVALID
 * before anything is launched, in this order: a NULL pointer; K outside 1..16 or n_verts outside 1..2^31-1; n_faces other than the raytracer's
 * triangle count; map_h or map_w outside 1..16384; n_freqs other than 12; a map or xin that is not 16-byte aligned; sdf_scale, uv_rate or
 * h_threshold not positive and finite; sdf_offset not finite.  (N == 0 returns NERFTEX_OK behind these; N above 2^31 - 1 -- two lanes per
 * point -- is refused last.)
 *
 * nerftex_curved_shape_infer: the whole no-grad forward as ONE call under the rows contract of nerftex_curved_field_infer --
 *   neighbour search (K) -> shape lookup -> sigma net -> trunc_exp / reflected view direction / SH -> colour net -> sigmoid + mask,
 * six launches (the last four are nerftex_curved_field_infer's own), nothing allocated, capturable.  The mid kernel normalises the coarse
 * normal (eval bit 1).
 *   rows >= live                      no work; sigma / rgbs keep what they held.
 *   live rows the march marked unused no search, no traversal, no texel read; sigma = 0, rgbs = 0.
 *   every other live row              bit for bit what nerftex_knn_query, nerftex_shape_lookup, nerftex_ffmlp_inference,
 *                                     nerftex_curved_mid_forward, nerftex_ffmlp_inference and nerftex_curved_out_forward give one after
 *                                     the other, widened to fp32 (a row with a non-finite normal: sigma = 0, rgbs = 0 through its mask).
 * NERFTEX_ERR_INVALID before anything is launched, in this order: a NULL descriptor; B % 128 != 0; n_verts outside 1..2^31-1; K outside 1..16;
 * n_features other than 16 or other network shapes than sigma net 48 / 32 / 2 / 16, colour net 32 / 64 / 3 / 3; a NULL raytracer or n_faces
 * other than its triangle count; the map extents, n_freqs, map alignment, scales and offset as above; (B == 0 returns NERFTEX_OK here;) a NULL
 * pointer, a scratch that is not 256-byte aligned or smaller than nerftex_curved_shape_infer_scratch_bytes(B); a weight vector that is not
 * 16-byte aligned.
 * ------------------------------------------------------------------------- */
int nerftex_shape_lookup(const nerftex_raytracer* rt, const float* xyz, const int32_t* knn_idx, const float* knn_dist, uint32_t N, uint32_t K,
                         const float* mesh_vertices, const float* vertex_normals, uint32_t n_verts, const float* face_uv, uint32_t n_faces,
                         const float* map, uint32_t map_h, uint32_t map_w, float sdf_scale, float sdf_offset, float uv_rate, float h_threshold,
                         uint32_t n_freqs, float* p_uv, float* sdf, uint8_t* mask, float* normal, int64_t* face_idx, void* xin, void* stream);
typedef struct nerftex_curved_shape_infer_desc {
    const nerftex_knn* knn;            /* the NEW mesh's neighbour grid                                                           */
    const nerftex_raytracer* tracer;   /* the NEW mesh's BVH                                                                      */
    const float* xyz;                  /* [B,3] sample positions                                                                  */
    const float* dirs;                 /* [B,3] view directions; dirs[row][0] > 1e29 marks an unused slot                         */
    uint32_t B;
    uint32_t n_verts;
    const float* mesh_vertices;        /* [n_verts,3]                                                                             */
    const float* vertex_normals;       /* [n_verts,3]                                                                             */
    const float* face_uv;              /* [n_faces,6]                                                                             */
    uint32_t n_faces;
    uint32_t K;                        /* neighbours per point (K_for_uv)                                                         */
    const float* map;                  /* [map_h, map_w, n_features] fp32, 16-byte aligned                                        */
    uint32_t map_h, map_w, n_features;
    float sdf_scale, sdf_offset, uv_rate, h_threshold;
    uint32_t n_freqs;                  /* FreqEncoder(height) bands (multires)                                                    */
    const void* sigma_weights;         /* fp16, 16-byte aligned                                                                   */
    uint32_t sigma_in, sigma_hidden, sigma_layers, sigma_out;
    const void* color_weights;         /* fp16, 16-byte aligned                                                                   */
    uint32_t color_in, color_hidden, color_layers, color_out;
    float fc_weight;
    int eval;                          /* the eval bits of nerftex_curved_mid_forward                                             */
    float* sigma;                      /* [B] fp32                                                                                */
    float* rgbs;                       /* [B,3] fp32                                                                              */
    const int32_t* units_dev;
    uint32_t rows_per_unit;
    void* scratch;                     /* caller-owned, 256-byte aligned, >= nerftex_curved_shape_infer_scratch_bytes(B) bytes    */
    size_t scratch_bytes;
} nerftex_curved_shape_infer_desc;
size_t nerftex_curved_shape_infer_scratch_bytes(uint32_t B);
int nerftex_curved_shape_infer(const nerftex_curved_shape_infer_desc* d, void* stream);

/* -------------------------------------------------------------------------
 * Extension: the field BAKED ONTO THE VERTICES of a fine mesh -- the `imported_type == 'unhash'` branch of MeshFeatureField.forward
 * (tools/map.py:708-714) over knn() with its defaults on the field's OWN mesh (:454-501: K neighbours, use_dir_vec, Shepard weights -- the normal
 * nerftex_curved_project computes, the same expression tree) and barycentric_mapping on the FINE mesh (:503-528).  One launch behind the
 * neighbour search (nerftex_knn_query over the field's own vertices).  Per sample x, all fp32; behind the normal every operation rounds on its own
 * (no fused multiply-add but the tracer's own o + t d):
 *   normal = nerftex_curved_project's coarse normal                          knn_idx: -1 is the last vertex, anything else is clamped
 *   d1, d2 = the closest hits on the fine mesh along +normal and -normal (10 on a miss); inner = d1 < d2; the nearer hit's face (-1 when both miss)
 *   sdf    = (inner ? -d1 : d2) / sdf_scale - sdf_offset                     (a true division; the caller clamps sdf_scale to >= 1e-5)
 *   mask   = |sdf| < min(9.5, h_threshold) and face != -1
 *   b      = (|p1 x p2|, |p2 x p0|, |p0 x p1|) / (their sum + 1e-5),  p_k = corner_k - p_sur        (face -1 reads face 0 under mask = 0)
 *   feature_c = (b0 f0c + b1 f1c) + b2 f2c,  f_k = vertex_features[face_vertices[face][k]]
 *   xin [N,48] fp16 = [half(features) | half(FreqEncoder(sdf)) | 1 x 7]
 * The reference's query_tbn(x) of :711 is dead work (nothing reads the tuple it returns) and is not done.
 * face_vertices [n_faces,3]: the corners' vertex ids by ORIGINAL face id, corner k being corner k of the triangle the raytracer was built from.  Every
 * id must lie in [0, n_fine_verts): the kernel does not clamp them, the caller checks the table once when it is made.  The corners' positions are read
 * from the raytracer's own triangle records, which hold fine_vertices[face_vertices[face]] as fp32: fine_vertices [n_fine_verts,3] is the array
 * the raytracer was built from and is not dereferenced.
 * nerftex_vertex_lookup is the plain form: any N, every row; bary [N,3].  NERFTEX_ERR_INVALID before anything is launched, in this order: a NULL
 * pointer; K outside 1..16; n_verts, then n_fine_verts, outside 1..2^31-1; n_faces other than the raytracer's triangle count; n_freqs other than 12;
 * vertex_features or xin not 16-byte aligned; sdf_scale or h_threshold not positive and finite; sdf_offset not finite.  (N == 0 returns NERFTEX_OK
 * behind these; N above 2^31 - 1 -- two lanes per point -- is refused last.)
 *
 * nerftex_curved_unhash_infer: the whole no-grad forward as ONE call under the rows contract of nerftex_curved_field_infer --
 *   neighbour search (K, the field's own grid) -> vertex lookup -> sigma net -> trunc_exp / reflected view direction / SH -> colour net -> sigmoid + mask,
 * six launches (the last four are nerftex_curved_field_infer's own), nothing allocated, capturable.  The mid kernel normalises the coarse
 * normal (eval bit 1).
 *   rows >= live                      no work; sigma / rgbs keep what they held.
 *   live rows the march marked unused no search, no traversal, no row read; sigma = 0, rgbs = 0.
 *   every other live row              bit for bit what nerftex_knn_query, nerftex_vertex_lookup, nerftex_ffmlp_inference,
 *                                     nerftex_curved_mid_forward, nerftex_ffmlp_inference and nerftex_curved_out_forward give one after
 *                                     the other, widened to fp32.
 * NERFTEX_ERR_INVALID before anything is launched, in this order: a NULL descriptor; B % 128 != 0; n_verts outside 1..2^31-1; K outside 1..16;
 * n_features other than 16 or other network shapes than sigma net 48 / 32 / 2 / 16, colour net 32 / 64 / 3 / 3; a NULL raytracer or n_faces
 * other than its triangle count; n_fine_verts, n_freqs, alignment, scale, threshold and offset as above; (B == 0 returns NERFTEX_OK here;) a NULL
 * pointer, a scratch that is not 256-byte aligned or smaller than nerftex_curved_unhash_infer_scratch_bytes(B); a weight vector that is not
 * 16-byte aligned.
 * ------------------------------------------------------------------------- */
int nerftex_vertex_lookup(const nerftex_raytracer* rt_fine, const float* xyz, const int32_t* knn_idx, const float* knn_dist, uint32_t N, uint32_t K,
                          const float* mesh_vertices, const float* vertex_normals, uint32_t n_verts, float dir_vec_wdist, /* the field's OWN mesh */
                          const float* fine_vertices, uint32_t n_fine_verts, const int32_t* face_vertices, uint32_t n_faces,
                          const float* vertex_features,                                                                   /* [n_fine_verts,16] fp32 */
                          float sdf_scale, float sdf_offset, float h_threshold, uint32_t n_freqs, float* sdf, uint8_t* mask, float* normal,
                          int64_t* face_idx, float* bary, void* xin, void* stream);
typedef struct nerftex_curved_unhash_infer_desc {
    const nerftex_knn* knn;            /* the field's OWN mesh's neighbour grid                                                   */
    const nerftex_raytracer* tracer;   /* the FINE mesh's BVH                                                                     */
    const float* xyz;                  /* [B,3] sample positions                                                                  */
    const float* dirs;                 /* [B,3] view directions; dirs[row][0] > 1e29 marks an unused slot                         */
    uint32_t B;
    uint32_t n_verts;
    const float* mesh_vertices;        /* [n_verts,3], the field's own mesh                                                       */
    const float* vertex_normals;       /* [n_verts,3]                                                                             */
    uint32_t K;                        /* neighbours per point                                                                    */
    float dir_vec_wdist;
    const float* fine_vertices;        /* [n_fine_verts,3], what the raytracer was built from                                     */
    uint32_t n_fine_verts;
    const int32_t* face_vertices;      /* [n_faces,3]                                                                             */
    uint32_t n_faces;
    const float* vertex_features;      /* [n_fine_verts, n_features] fp32, 16-byte aligned                                        */
    uint32_t n_features;
    float sdf_scale, sdf_offset, h_threshold;
    uint32_t n_freqs;                  /* FreqEncoder(height) bands (multires)                                                    */
    const void* sigma_weights;         /* fp16, 16-byte aligned                                                                   */
    uint32_t sigma_in, sigma_hidden, sigma_layers, sigma_out;
    const void* color_weights;         /* fp16, 16-byte aligned                                                                   */
    uint32_t color_in, color_hidden, color_layers, color_out;
    float fc_weight;
    int eval;                          /* the eval bits of nerftex_curved_mid_forward                                             */
    float* sigma;                      /* [B] fp32                                                                                */
    float* rgbs;                       /* [B,3] fp32                                                                              */
    const int32_t* units_dev;
    uint32_t rows_per_unit;
    void* scratch;                     /* caller-owned, 256-byte aligned, >= nerftex_curved_unhash_infer_scratch_bytes(B) bytes   */
    size_t scratch_bytes;
} nerftex_curved_unhash_infer_desc;
size_t nerftex_curved_unhash_infer_scratch_bytes(uint32_t B);
int nerftex_curved_unhash_infer(const nerftex_curved_unhash_infer_desc* d, void* stream);

/* -------------------------------------------------------------------------
 * Extension: the same ONE call for the curved field with the SH light model (CurvedField(light_model="SH")), under the same rows contract:
 *   neighbour search -> projector (+ the hit face's frame) -> hash-grid gather of the texture table -> gather of the normal net's table ->
 *   sigma net 48 -> 32 -> 16 -> light mid: exp / BRDF input / the factorized fine-normal net (two 16-wide LipMLPs, toCoor, the frame's
 *   rotation, the normalisations, in eval the fc_weight blend with the coarse normal) -> BRDF net 16 -> 64 x 3 -> 16 -> light out: the SH
 *   light head (the row function of nerftex_sh_light_forward) + the height mask,
 * ten launches enqueued on `stream`; nothing is allocated, the host never waits, the call can be captured.
 *   rows >= live                      no work; sigma / rgbs / shading_normal keep what they held.
 *   live rows the march marked unused no search, no traversal, no table read; sigma = 0, rgbs = 0, shading_normal = 0.
 *   every other live row              sigma = mask ? exp(h[:, 0]) : 0 in fp32 (what the field's forward() gives, bit for bit);
 *                                     rgbs = mask ? the output visual_mode selects : 0;  shading_normal = the normal the head shades with.
 * The normal net's arithmetic at the framework's rounding points under fp16 autocast: every LipLayer product W_n x is a half GEMM (inputs and
 * normalised weights half, fp32 accumulation in ascending input order, the result rounded to half), bias and ReLU fp32, the next layer rounds
 * to half again; the rotation by the face frame is a half product too; everything else fp32, every operation rounded on its own.
 * normal_weights: the six normalised weight matrices as fp16, row-major [out, in], one after the other -- phi net [16,20] [16,16] [1,16] (inputs:
 * the 8 features of the normal table, then the first 12 height bands), theta net [16,28] [16,16] [1,16] (inputs: the first 16 texture features,
 * then the same 12 bands): NERFTEX_NORMAL_NET_WEIGHTS values; normal_biases: their fp32 biases in the same order, NERFTEX_NORMAL_NET_BIASES values.
 * NERFTEX_ERR_INVALID with a message, before anything is launched, in this order: a NULL descriptor; B % 128 != 0; n_verts, K or a shape other
 * than the default SH field's (n_freqs 12; texture table 3-D, 2 x 8; normal table 2 x 4; sigma net 48 / 32 / 2 / 16; normal nets 16 wide with 2
 * hidden layers; BRDF net 16 / 64 / 3 / 5; n_sh >= 9, n_color 1 or 3, gamma positive and finite, flags, visual_mode, eval 0 or 1); then
 * B == 0 returns NERFTEX_OK; then NULL handles / buffers, alignment, a scratch smaller than nerftex_curved_light_infer_scratch_bytes(B).
 * ------------------------------------------------------------------------- */
#define NERFTEX_LIGHT_VISUAL_FULL 0
#define NERFTEX_LIGHT_VISUAL_SPECULAR 1
#define NERFTEX_LIGHT_VISUAL_DIFFUSE 2
#define NERFTEX_LIGHT_VISUAL_ALBEDO 3
#define NERFTEX_NORMAL_NET_WEIGHTS 1312 /* 16 x 20 + 16 x 16 + 16 + 16 x 28 + 16 x 16 + 16 */
#define NERFTEX_NORMAL_NET_BIASES 66    /* 16 + 16 + 1 + 16 + 16 + 1                       */
typedef struct nerftex_curved_light_infer_desc {
    const nerftex_knn* knn;            /* as nerftex_curved_infer_desc, down to in_mul                                            */
    const nerftex_raytracer* tracer;
    const float* xyz;
    const float* dirs;
    uint32_t B;
    uint32_t n_verts;
    const float* mesh_vertices;
    const float* vertex_normals;
    const float* tbn;                  /* [F,9] per-face frames (rows t, b, n): read for the hit face of every unmarked live row   */
    uint32_t K;
    uint32_t n_freqs;
    float dir_vec_wdist;
    float h_threshold;
    const void* table;
    const int32_t* offsets;
    uint32_t D, C, L;
    float S;
    uint32_t H;
    uint32_t gridtype;
    int align_corners;
    float in_add, in_mul;
    const void* normal_table;          /* the normal net's own fp16 hash table [rows, normal_C], read at the same surface point    */
    const int32_t* normal_offsets;     /* [normal_L + 1] (device)                                                                 */
    uint32_t normal_C, normal_L;       /* 2 features x 4 levels                                                                   */
    float normal_S;
    uint32_t normal_H;
    uint32_t normal_gridtype;
    int normal_align_corners;
    float normal_in_add, normal_in_mul;
    const void* sigma_weights;         /* fp16, 16-byte aligned                                                                   */
    uint32_t sigma_in, sigma_hidden, sigma_layers, sigma_out;
    const void* normal_weights;        /* fp16 [NERFTEX_NORMAL_NET_WEIGHTS], 4-byte aligned: see above                            */
    const float* normal_biases;        /* fp32 [NERFTEX_NORMAL_NET_BIASES]                                                        */
    uint32_t normal_hidden, normal_layers; /* 16, 2                                                                               */
    const void* brdf_weights;          /* fp16, 16-byte aligned                                                                   */
    uint32_t brdf_in, brdf_hidden, brdf_layers, brdf_out;
    const float* env_shs;              /* [n_sh, n_color] fp32, as nerftex_sh_light_desc                                          */
    uint32_t n_sh, n_color;
    float gamma;
    uint32_t flags;                    /* NERFTEX_SH_LIGHT_SPECULAR                                                               */
    uint32_t visual_mode;              /* NERFTEX_LIGHT_VISUAL_*: which of the head's four outputs rgbs receives                  */
    float fc_weight;
    int eval;                          /* 1: the shading normal is fc_weight x fine + (1 - fc_weight) x coarse, renormalised; 0: the fine normal */
    float* sigma;                      /* [B] fp32                                                                                */
    float* rgbs;                       /* [B,3] fp32                                                                              */
    float* shading_normal;             /* [B,3] fp32 or NULL (not written)                                                        */
    const int32_t* units_dev;
    uint32_t rows_per_unit;
    void* scratch;                     /* caller-owned, 256-byte aligned, >= nerftex_curved_light_infer_scratch_bytes(B) bytes    */
    size_t scratch_bytes;
} nerftex_curved_light_infer_desc;
size_t nerftex_curved_light_infer_scratch_bytes(uint32_t B);
int nerftex_curved_light_infer(const nerftex_curved_light_infer_desc* d, void* stream);

/* -------------------------------------------------------------------------
 * Extension: the IMPORTED planar map under the SH light model -- the `pred_normal` part of the 'field' branch of MeshFeatureField.forward
 * (tools/map.py:670-675, :722-730).  Beside the [map_h, map_w, 16] feature map of nerftex_planar_lookup, three more device arrays:
 *   phi_map        [map_h, map_w, 8] fp32: the normal net's own table features per texel, read BILINEARLY with the feature read's expression.
 *   frame_map      [map_h, map_w, 12] fp32: per texel three 16-byte words -- the 9 floats of its frame (`local_tbn`, row-major 3 x 3), its patch
 *                  id as a float (`sample_tbn_ids`), two zeros.  Read NEAREST: ix = ((u + 1) / 2) (map_h - 1) in fp32, rounded half to even
 *                  (nearbyintf), iy likewise; a texel index outside the map gives zeros (frame 0, id 0); the id is the float truncated.
 *   sample_tbn_inv [n_patches, 12] fp32: the 9 floats of each patch's INVERTED frame, three zeros; row `id` is read.  An id outside
 *                  [0, n_patches) -- the caller rules it out -- reads nothing: zeros, and patch_id = -1 in the plain form.
 * All four maps in the axis order MeshFeatureField.import_field receives: u runs along the first axis.
 * nerftex_planar_light_lookup is the plain form (any B, every row): p_uv, sdf, mask, xin bit for bit nerftex_planar_lookup's; phi [B,8] fp32 (the
 * rows form narrows exactly these values to half); patch_id [B] int32; local_tbn [B,9] and sample_tbn [B,9] fp32.  Refusals, in this order:
 * n_freqs other than 12; map_h or map_w outside 1..16384; n_patches outside 1..2^24; (B == 0 returns NERFTEX_OK here;) a NULL pointer, a map,
 * the patch frames, xin or phi not 16-byte aligned; mode, scales, h_threshold, sdf_offset as nerftex_planar_lookup.
 *
 * nerftex_curved_light_import_infer: the lit field's whole no-grad forward over these maps as ONE call under the rows contract of
 * nerftex_curved_light_infer, five launches, nothing allocated, capturable --
 *   lit lookup -> sigma net 48 -> 32 -> 16 -> light mid (the normal net fed from phi_map; the local normal rotated by the texel's frame and
 *   then by the patch's inverted frame, two half products one after the other, each result rounded to half -- the frames are NOT multiplied
 *   together; the two normalisations; in eval the fc_weight blend with the coarse normal (0, 0, 1)) -> BRDF net 16 -> 64 x 3 -> 16 -> light out.
 *   rows >= live                      no work; sigma / rgbs / shading_normal keep what they held.
 *   live rows the march marked unused no texel of any map is read; sigma = 0, rgbs = 0, shading_normal = 0.
 *   every other live row              sigma and the mask bit for bit the field's forward(); rgbs, shading_normal as nerftex_curved_light_infer.
 * NERFTEX_ERR_INVALID with a message, before anything is launched, in this order: a NULL descriptor; B % 128 != 0; n_features other than 16,
 * n_phi other than 8, n_freqs other than 12 or other network shapes than the default SH field's; n_sh, n_color, gamma, flags, visual_mode, eval
 * as nerftex_curved_light_infer; map_h or map_w outside 1..16384; n_patches outside 1..2^24; (B == 0 returns NERFTEX_OK here;) a NULL pointer,
 * a scratch that is not 256-byte aligned or smaller than nerftex_curved_light_import_infer_scratch_bytes(B); a map, the patch frames or an MLP
 * weight vector not 16-byte aligned, the normal net's block not 4-byte aligned; mode, scales, h_threshold, sdf_offset as nerftex_planar_lookup.
 * ------------------------------------------------------------------------- */
#define NERFTEX_FRAME_MAP_STRIDE 12 /* floats per texel of frame_map and per row of sample_tbn_inv */
int nerftex_planar_light_lookup(const float* xyz, const float* map, const float* phi_map, const float* frame_map, const float* sample_tbn_inv,
                                uint32_t map_h, uint32_t map_w, uint32_t n_patches, uint32_t mode, float plane_scale0, float plane_scale1,
                                float height_scale0, float height_scale1, float sdf_offset, float h_threshold, uint32_t n_freqs, uint32_t B, float* p_uv,
                                float* sdf, uint8_t* mask, void* xin, float* phi, int32_t* patch_id, float* local_tbn, float* sample_tbn, void* stream);
typedef struct nerftex_curved_light_import_infer_desc {
    const float* xyz;                  /* [B,3] sample positions                                                                  */
    const float* dirs;                 /* [B,3] view directions; dirs[row][0] > 1e29 marks an unused slot                         */
    uint32_t B;
    const float* map;                  /* [map_h, map_w, n_features] fp32, 16-byte aligned                                        */
    const float* phi_map;              /* [map_h, map_w, n_phi] fp32, 16-byte aligned                                             */
    const float* frame_map;            /* [map_h, map_w, NERFTEX_FRAME_MAP_STRIDE] fp32, 16-byte aligned: see above               */
    const float* sample_tbn_inv;       /* [n_patches, NERFTEX_FRAME_MAP_STRIDE] fp32, 16-byte aligned: see above                  */
    uint32_t map_h, map_w, n_features, n_phi, n_patches;
    uint32_t mode;                     /* NERFTEX_PLANAR_MULTIPLY / NERFTEX_PLANAR_DIVIDE                                          */
    float plane_scale0, plane_scale1;
    float height_scale0, height_scale1;
    float sdf_offset;
    float h_threshold;
    uint32_t n_freqs;                  /* FreqEncoder(height) bands (multires)                                                    */
    const void* sigma_weights;         /* fp16, 16-byte aligned                                                                   */
    uint32_t sigma_in, sigma_hidden, sigma_layers, sigma_out;
    const void* normal_weights;        /* fp16 [NERFTEX_NORMAL_NET_WEIGHTS], 4-byte aligned: as nerftex_curved_light_infer_desc   */
    const float* normal_biases;        /* fp32 [NERFTEX_NORMAL_NET_BIASES]                                                        */
    uint32_t normal_hidden, normal_layers; /* 16, 2                                                                               */
    const void* brdf_weights;          /* fp16, 16-byte aligned                                                                   */
    uint32_t brdf_in, brdf_hidden, brdf_layers, brdf_out;
    const float* env_shs;              /* [n_sh, n_color] fp32, as nerftex_sh_light_desc                                          */
    uint32_t n_sh, n_color;
    float gamma;
    uint32_t flags;                    /* NERFTEX_SH_LIGHT_SPECULAR                                                               */
    uint32_t visual_mode;              /* NERFTEX_LIGHT_VISUAL_*                                                                  */
    float fc_weight;
    int eval;                          /* as nerftex_curved_light_infer_desc                                                      */
    float* sigma;                      /* [B] fp32                                                                                */
    float* rgbs;                       /* [B,3] fp32                                                                              */
    float* shading_normal;             /* [B,3] fp32 or NULL (not written)                                                        */
    const int32_t* units_dev;
    uint32_t rows_per_unit;
    void* scratch;                     /* caller-owned, 256-byte aligned, >= nerftex_curved_light_import_infer_scratch_bytes(B)   */
    size_t scratch_bytes;
} nerftex_curved_light_import_infer_desc;
size_t nerftex_curved_light_import_infer_scratch_bytes(uint32_t B);
int nerftex_curved_light_import_infer(const nerftex_curved_light_import_infer_desc* d, void* stream);

/* -------------------------------------------------------------------------
 * Extension: the imported maps on a NEW UV-MAPPED MESH under the SH light model -- the `pred_normal` part of the 'shape' branch of
 * MeshFeatureField.forward (tools/map.py:693-707, :722-730): nerftex_shape_lookup's work for one sample, plus, at the row's own (u, v), the lit
 * reads of nerftex_planar_light_lookup (the nearest frame texel, the patch frame that hangs on its id, the bilinear phi read), plus the hit
 * face's frame new_tbn = face_tbn[face] (:542; face -1, a double miss, reads face 0 as the reference does -- its mask is 0).
 *   face_tbn [n_tbn_faces, NERFTEX_FRAME_MAP_STRIDE] fp32, 16-byte aligned, indexed by the ORIGINAL face id (not the BVH's order): the 9 floats
 *   of the face's frame (rows t, b, n of calculate_tbn, :119-138, over the normalised mesh and the [-1, 1] UVs), three zeros.
 * One launch behind the neighbour search, two lanes per point as nerftex_shape_lookup: the (u, v)-dependent reads sit on the lane that reads the
 * features, the face frame on the lane that writes the height ladder.  No rounding point is new: the values are the two lookups' own.
 * A row whose normal is not finite reads no face, UV, frame or texel of any map: nerftex_shape_lookup's constants, and zeros for phi and all
 * three frames, patch_id = -1.
 * nerftex_shape_light_lookup is the plain form (any N, every row): p_uv, sdf, mask, normal, face_idx, xin bit for bit nerftex_shape_lookup's;
 * phi [N,8] fp32 (the rows form narrows exactly these values to half); patch_id [N] int32; local_tbn, sample_tbn, new_tbn [N,9] fp32.
 * NERFTEX_ERR_INVALID before anything is launched, in this order: nerftex_shape_lookup's refusals over the arguments the two share (a NULL
 * pointer; K or n_verts; n_faces other than the raytracer's triangle count; map extents; n_freqs; alignment of the map and of xin; scales,
 * threshold; offset); then nerftex_planar_light_lookup's over what this entry adds (n_patches outside 1..2^24; a NULL lit map, patch frames,
 * face_tbn or lit output; a lit map, the patch frames, face_tbn or phi not 16-byte aligned); then n_tbn_faces other than the raytracer's
 * triangle count.  (N == 0 returns NERFTEX_OK behind these; N above 2^31 - 1 is refused last.)
 *
 * nerftex_curved_light_shape_infer: the lit field's whole no-grad forward over the maps on the new mesh as ONE call under the rows contract of
 * nerftex_curved_light_infer, six launches, nothing allocated, capturable --
 *   neighbour search (K) -> lit shape lookup -> sigma net 48 -> 32 -> 16 -> light mid (the normal net fed from phi_map; the local normal rotated
 *   by the texel's frame, then by the patch's inverted frame, then by the new mesh's face frame: three half products one after the other, each
 *   result rounded to half -- the frames are NEVER multiplied together; the two normalisations; in eval the fc_weight blend with the coarse
 *   normal of the new mesh) -> BRDF net 16 -> 64 x 3 -> 16 -> light out.
 *   rows >= live                      no work; sigma / rgbs / shading_normal keep what they held.
 *   live rows the march marked unused no search, no traversal, no texel of any map; sigma = 0, rgbs = 0, shading_normal = 0.
 *   every other live row              sigma and the mask bit for bit the field's forward(); rgbs, shading_normal as nerftex_curved_light_infer.
 * NERFTEX_ERR_INVALID with a message, before anything is launched, in this order: a NULL descriptor; B % 128 != 0; n_verts outside 1..2^31-1;
 * K outside 1..16; n_features other than 16, n_phi other than 8 or other network shapes than the default SH field's; n_sh, n_color, gamma,
 * flags, visual_mode, eval as nerftex_curved_light_infer; a NULL raytracer or n_faces other than its triangle count; the map extents, n_freqs,
 * map alignment, scales and offset as nerftex_shape_lookup; n_patches outside 1..2^24; n_tbn_faces other than n_faces; (B == 0 returns
 * NERFTEX_OK here;) a NULL pointer, a scratch that is not 256-byte aligned or smaller than nerftex_curved_light_shape_infer_scratch_bytes(B);
 * a lit map, the patch frames, face_tbn or an MLP weight vector not 16-byte aligned, the normal net's block not 4-byte aligned.
 * ------------------------------------------------------------------------- */
int nerftex_shape_light_lookup(const nerftex_raytracer* rt, const float* xyz, const int32_t* knn_idx, const float* knn_dist, uint32_t N, uint32_t K,
                               const float* mesh_vertices, const float* vertex_normals, uint32_t n_verts, const float* face_uv, uint32_t n_faces,
                               const float* face_tbn, uint32_t n_tbn_faces, const float* map, const float* phi_map, const float* frame_map,
                               const float* sample_tbn_inv, uint32_t map_h, uint32_t map_w, uint32_t n_patches, float sdf_scale, float sdf_offset,
                               float uv_rate, float h_threshold, uint32_t n_freqs, float* p_uv, float* sdf, uint8_t* mask, float* normal,
                               int64_t* face_idx, void* xin, float* phi, int32_t* patch_id, float* local_tbn, float* sample_tbn, float* new_tbn,
                               void* stream);
typedef struct nerftex_curved_light_shape_infer_desc {
    const nerftex_knn* knn;            /* the NEW mesh's neighbour grid                                                           */
    const nerftex_raytracer* tracer;   /* the NEW mesh's BVH                                                                      */
    const float* xyz;                  /* [B,3] sample positions                                                                  */
    const float* dirs;                 /* [B,3] view directions; dirs[row][0] > 1e29 marks an unused slot                         */
    uint32_t B;
    uint32_t n_verts;
    const float* mesh_vertices;        /* [n_verts,3]                                                                             */
    const float* vertex_normals;       /* [n_verts,3]                                                                             */
    const float* face_uv;              /* [n_faces,6]                                                                             */
    const float* face_tbn;             /* [n_tbn_faces, NERFTEX_FRAME_MAP_STRIDE] fp32, 16-byte aligned: see above                */
    uint32_t n_faces, n_tbn_faces;
    uint32_t K;                        /* neighbours per point (K_for_uv)                                                         */
    const float* map;                  /* [map_h, map_w, n_features] fp32, 16-byte aligned                                        */
    const float* phi_map;              /* [map_h, map_w, n_phi] fp32, 16-byte aligned                                             */
    const float* frame_map;            /* [map_h, map_w, NERFTEX_FRAME_MAP_STRIDE] fp32, 16-byte aligned                          */
    const float* sample_tbn_inv;       /* [n_patches, NERFTEX_FRAME_MAP_STRIDE] fp32, 16-byte aligned                             */
    uint32_t map_h, map_w, n_features, n_phi, n_patches;
    float sdf_scale, sdf_offset, uv_rate, h_threshold;
    uint32_t n_freqs;                  /* FreqEncoder(height) bands (multires)                                                    */
    const void* sigma_weights;         /* fp16, 16-byte aligned                                                                   */
    uint32_t sigma_in, sigma_hidden, sigma_layers, sigma_out;
    const void* normal_weights;        /* fp16 [NERFTEX_NORMAL_NET_WEIGHTS], 4-byte aligned: as nerftex_curved_light_infer_desc   */
    const float* normal_biases;        /* fp32 [NERFTEX_NORMAL_NET_BIASES]                                                        */
    uint32_t normal_hidden, normal_layers; /* 16, 2                                                                               */
    const void* brdf_weights;          /* fp16, 16-byte aligned                                                                   */
    uint32_t brdf_in, brdf_hidden, brdf_layers, brdf_out;
    const float* env_shs;              /* [n_sh, n_color] fp32, as nerftex_sh_light_desc                                          */
    uint32_t n_sh, n_color;
    float gamma;
    uint32_t flags;                    /* NERFTEX_SH_LIGHT_SPECULAR                                                               */
    uint32_t visual_mode;              /* NERFTEX_LIGHT_VISUAL_*                                                                  */
    float fc_weight;
    int eval;                          /* as nerftex_curved_light_infer_desc                                                      */
    float* sigma;                      /* [B] fp32                                                                                */
    float* rgbs;                       /* [B,3] fp32                                                                              */
    float* shading_normal;             /* [B,3] fp32 or NULL (not written)                                                        */
    const int32_t* units_dev;
    uint32_t rows_per_unit;
    void* scratch;                     /* caller-owned, 256-byte aligned, >= nerftex_curved_light_shape_infer_scratch_bytes(B)    */
    size_t scratch_bytes;
} nerftex_curved_light_shape_infer_desc;
size_t nerftex_curved_light_shape_infer_scratch_bytes(uint32_t B);
int nerftex_curved_light_shape_infer(const nerftex_curved_light_shape_infer_desc* d, void* stream);

/* -------------------------------------------------------------------------
 * Extension: the front of the patch export -- the per-candidate part of MeshFeatureField.sample_patches (tools/map.py:1030-1084, the
 * non-trimesh path) for a CHUNK of B candidate patches of S x S pixels in three launches and no host synchronisation, instead of one
 * 16 384-ray trace, one CPU KD-tree query and one read-back per candidate.
 *   cast    grid (ceil(S^2 / 64), B), one pixel per lane.  Pixel p = i S + j has the local coordinates (x, y) = (calibration[i],
 *           calibration[j]) (meshgrid(indexing='ij')).  With T = frames[b] ([3,4] row-major: columns x axis, y axis, z axis, centre), per axis a
 *               o[a]      = (T[a][0] x + T[a][1] y) + T[a][3]      the pre-lift origin: every product and sum rounded on its own (fp32,
 *                                                                  no fused multiply-add); the reference's T[a][2] * 0 term is dropped
 *               origin[a] = o[a] + (0.1f T[a][2]),  direction[a] = -T[a][2]
 *           and the ray is traced as nerftex_raytracer_trace traces it (intersection = fma(depth, direction, origin); depth 10 on a miss).
 *           origins [B,S^2,3] takes the PRE-LIFT origins, intersections [B,S^2,3] the hits, rays [B,S^2,6] (optional) the lifted origin and
 *           the direction.  Per patch: the maximum depth and "a pre-lift origin is NaN", reduced per wave, one vector atomic per wave.
 *   scan    only with a scan cloud: the distance of every pre-lift origin to its nearest scan point (nerftex_knn_query's search with K = 1,
 *           its distance bit for bit) and per patch the maximum.
 *   select  one workgroup.  verdict[b], in the reference's order of tests -- 2: a NaN origin; 3: maximum scan distance > max_scan_dist;
 *           4: maximum depth > 9.5 (a ray missed); 0: accepted -- and 5 for EVERY candidate behind the one that made the running count reach
 *           max_patch_num (the reference's loop has ended there).  count[0] is the device-resident number of patches accepted so far (the caller zeroes
 *           it once); slot[b] = the global patch index of an accepted candidate (count[0] before the call + its rank among the chunk's accepted,
 *           in candidate order), -1 otherwise; count[0] grows by the number accepted.  (Code 1, "below y = 0 with no scan cloud", is the host's.)
 * stats [B,4] uint32 is scratch (zeroed by the call): {bits of the maximum depth, NaN flag, bits of the maximum scan distance, 0}.
 * NERFTEX_ERR_INVALID before anything touches a device: a NULL descriptor or tracer, frames, calibration, origins, intersections, stats,
 * verdict, slot or count; B = 0; S = 0; S^2 B beyond uint32; max_patch_num = 0.
 * ------------------------------------------------------------------------- */
typedef struct nerftex_patch_front_desc {
    const nerftex_raytracer* tracer;   /* the mesh the patches are cast on                                                        */
    const nerftex_knn* scan;           /* the scan cloud's grid, or NULL: no scan test                                            */
    const float* frames;               /* [B,12] fp32: T[:3,:4] of every candidate, row-major                                     */
    const float* calibration;          /* [S] fp32                                                                                */
    uint32_t B, S;
    float max_scan_dist;               /* min(0.1, 3 h_threshold) of tools/map.py:1078                                            */
    uint32_t max_patch_num;
    float* origins;                    /* [B,S^2,3] fp32 out: the pre-lift origins                                                */
    float* intersections;              /* [B,S^2,3] fp32 out                                                                      */
    float* rays;                       /* [B,S^2,6] fp32 out, or NULL                                                             */
    uint32_t* stats;                   /* [B,4] scratch                                                                           */
    uint8_t* verdict;                  /* [B] out                                                                                 */
    int32_t* slot;                     /* [B] out                                                                                 */
    uint32_t* count;                   /* [1] in / out, device-resident                                                           */
} nerftex_patch_front_desc;
int nerftex_patch_front(const nerftex_patch_front_desc* d, void* stream);

/* -------------------------------------------------------------------------
 * Extension: an IMPORTED FEATURE PATCH under the curved field -- the `imported_type == 'patch'` branch of MeshFeatureField.forward
 * (tools/map.py:676-692) over MeshProjector.weighted_project(weighting='DualD') (:435-452) and knn(use_dir_vec=False, direct_above_check=True,
 * direct_above_threshold=1., weighting='Shepard') (:454-501): what NeRFNetwork.import_patch shows of one patch nerftex_patch_front's export
 * produced.  The patch is an oriented point cloud of V = n_points points; `knn` is a nerftex_knn_create grid over their positions.  Per-point
 * records, fp32, each array 16-byte aligned, row i = the point nerftex_knn_query calls i:
 *   geom     [V, NERFTEX_PATCH_GEOM_STRIDE = 8]   {px, py, pz, 0, nx, ny, nz, 0}
 *   features [V, 16]
 *   lit      [V, NERFTEX_PATCH_LIT_STRIDE = 20]   {phi_embed 0..7, local_tbn 0..8 (row-major 3 x 3), 0, 0, 0}      (the lit forms only)
 * Per sample x, all fp32, every operation rounded on its own (no fused multiply-add), sums in ascending k:
 *   idx_k, dis_k       nerftex_knn_query's K = 8 nearest points and Euclidean distances, bit for bit
 *   dv_k = x - p[idx_k],  dir_k = dv_k / (|dv_k| + 1e-5),  above = 2 min_k |n[idx_k] x dir_k| < 1
 *   not above:         every dis_k and every component of every dv_k becomes 1e5 (a select: the row goes on with these values)
 *   a_k = 1 / (dis_k + 1e-7),  a_k /= sum a;  normal = sum_k a_k n_k / (|n_k| + 1e-5),  normal /= |normal| + 1e-5
 *   s_k = dv_k . normal,  t_k = |(dv_k - s_k normal)^2|_2  (the 2-norm of the component-wise squares),  dk = max t, d1 = min t
 *   w_k = (((dk - t_k) / ((dk - d1) + 1e-5)) (dk + d1)) / (dk + t_k),  w_k /= sum w + 1e-5;  sdf = sum_k s_k w_k
 *   mask = |sdf| < h_threshold and dis_0 < h_threshold (both strict; dis_0, the smallest, AFTER the select)
 *   features = sum_k w_k features[idx_k];  lit: phi = sum_k w_k phi[idx_k], local_tbn = sum_k w_k tbn[idx_k]
 *   xin [B,48] fp16 = [half(features) | half(FreqEncoder(sdf)), 25 values | 1 x 7];  normal is the RAW coarse normal (normalised once)
 * A sample that is not finite gets NaNs and mask 0 (idx -1, nothing is read out of bounds).
 * nerftex_patch_lookup / nerftex_patch_light_lookup are the plain forms (any B, every row): sdf [B], mask [B] bytes, normal [B,3], xin, idx [B,8]
 * int32, dis [B,8] (before the select), weights [B,8] = w, and lit phi [B,8] fp32 and local_tbn [B,9].  NERFTEX_ERR_INVALID before anything is
 * launched, in this order: a NULL grid, an n_points that is not the grid's, below 8 or above 2^31 - 1; n_freqs other than 12; (B == 0 returns
 * NERFTEX_OK here;) a NULL input or output pointer, a phi that is not 16-byte aligned; a NULL record array; a record array or xin that is not
 * 16-byte aligned; an h_threshold that is not positive and finite.
 *
 * nerftex_curved_patch_infer / nerftex_curved_light_patch_infer: the whole no-grad forward over such a patch as ONE call under the rows contract
 * of nerftex_curved_field_infer --
 *   lookup (search + resampling, one kernel) -> sigma net -> [static] mid / colour net / sigmoid + mask   (nerftex_curved_import_infer's four)
 *                                                         -> [lit] light mid / BRDF net / head + mask      (nerftex_curved_light_infer's four:
 *                                                            ONE rotation, by the lookup's weighted local_tbn, a half product as there)
 * five launches, nothing allocated, capturable.
 *   rows >= live                      no work; sigma / rgbs keep what they held.
 *   live rows the march marked unused no search, no gather; sigma = 0, rgbs = 0.
 *   every other live row              bit for bit what the plain lookup and the pieces of nerftex_curved_import_infer /
 *                                     nerftex_curved_light_infer give one after the other.
 * NERFTEX_ERR_INVALID with a message, before anything is launched, in this order: a NULL descriptor; B % 128 != 0; a NULL grid, an n_points that
 * is not the grid's, below 8 or above 2^31 - 1; other shapes than 16 features (lit: 8 phi features), 12 height bands and the default networks;
 * (lit: the light head's refusals, as nerftex_curved_light_infer;) (B == 0 returns NERFTEX_OK here;) a NULL pointer, a scratch that is not
 * 256-byte aligned or smaller than the entry's _scratch_bytes(B); a weight vector that is not 16-byte aligned (lit: the normal net's block
 * 4-byte); a record array that is not 16-byte aligned; an h_threshold that is not positive and finite.
 * ------------------------------------------------------------------------- */
#define NERFTEX_PATCH_GEOM_STRIDE 8
#define NERFTEX_PATCH_LIT_STRIDE 20
int nerftex_patch_lookup(const nerftex_knn* knn, const float* xyz, const float* geom, const float* features, uint32_t n_points, float h_threshold,
                         uint32_t n_freqs, uint32_t B, float* sdf, uint8_t* mask, float* normal, void* xin, int32_t* idx, float* dis, float* weights,
                         void* stream);
int nerftex_patch_light_lookup(const nerftex_knn* knn, const float* xyz, const float* geom, const float* features, const float* lit, uint32_t n_points,
                               float h_threshold, uint32_t n_freqs, uint32_t B, float* sdf, uint8_t* mask, float* normal, void* xin, int32_t* idx,
                               float* dis, float* weights, float* phi, float* local_tbn, void* stream);
typedef struct nerftex_curved_patch_infer_desc {
    const nerftex_knn* knn;            /* the neighbour grid over the patch's points                                              */
    const float* xyz;                  /* [B,3] sample positions                                                                  */
    const float* dirs;                 /* [B,3] view directions; dirs[row][0] > 1e29 marks an unused slot                         */
    uint32_t B;
    uint32_t n_points;                 /* V: the grid's point count                                                               */
    const float* geom;                 /* [V, NERFTEX_PATCH_GEOM_STRIDE] fp32, 16-byte aligned                                    */
    const float* features;             /* [V, n_features] fp32, 16-byte aligned                                                   */
    uint32_t n_features;
    float h_threshold;
    uint32_t n_freqs;                  /* FreqEncoder(height) bands (multires)                                                    */
    const void* sigma_weights;         /* fp16, 16-byte aligned                                                                   */
    uint32_t sigma_in, sigma_hidden, sigma_layers, sigma_out;
    const void* color_weights;         /* fp16, 16-byte aligned                                                                   */
    uint32_t color_in, color_hidden, color_layers, color_out;
    float fc_weight;
    int eval;                          /* the eval bits of nerftex_curved_mid_forward                                             */
    float* sigma;                      /* [B] fp32                                                                                */
    float* rgbs;                       /* [B,3] fp32                                                                              */
    const int32_t* units_dev;
    uint32_t rows_per_unit;
    void* scratch;                     /* caller-owned, 256-byte aligned, >= nerftex_curved_patch_infer_scratch_bytes(B) bytes    */
    size_t scratch_bytes;
} nerftex_curved_patch_infer_desc;
size_t nerftex_curved_patch_infer_scratch_bytes(uint32_t B);
int nerftex_curved_patch_infer(const nerftex_curved_patch_infer_desc* d, void* stream);
typedef struct nerftex_curved_light_patch_infer_desc {
    const nerftex_knn* knn;            /* the neighbour grid over the patch's points                                              */
    const float* xyz;                  /* [B,3] sample positions                                                                  */
    const float* dirs;                 /* [B,3] view directions; dirs[row][0] > 1e29 marks an unused slot                         */
    uint32_t B;
    uint32_t n_points;                 /* V: the grid's point count                                                               */
    const float* geom;                 /* [V, NERFTEX_PATCH_GEOM_STRIDE] fp32, 16-byte aligned                                    */
    const float* features;             /* [V, n_features] fp32, 16-byte aligned                                                   */
    const float* lit;                  /* [V, NERFTEX_PATCH_LIT_STRIDE] fp32, 16-byte aligned                                     */
    uint32_t n_features, n_phi;
    float h_threshold;
    uint32_t n_freqs;                  /* FreqEncoder(height) bands (multires)                                                    */
    const void* sigma_weights;         /* fp16, 16-byte aligned                                                                   */
    uint32_t sigma_in, sigma_hidden, sigma_layers, sigma_out;
    const void* normal_weights;        /* fp16 [NERFTEX_NORMAL_NET_WEIGHTS], 4-byte aligned: as nerftex_curved_light_infer_desc   */
    const float* normal_biases;        /* fp32 [NERFTEX_NORMAL_NET_BIASES]                                                        */
    uint32_t normal_hidden, normal_layers; /* 16, 2                                                                               */
    const void* brdf_weights;          /* fp16, 16-byte aligned                                                                   */
    uint32_t brdf_in, brdf_hidden, brdf_layers, brdf_out;
    const float* env_shs;              /* [n_sh, n_color] fp32, as nerftex_sh_light_desc                                          */
    uint32_t n_sh, n_color;
    float gamma;
    uint32_t flags;                    /* NERFTEX_SH_LIGHT_SPECULAR                                                               */
    uint32_t visual_mode;              /* NERFTEX_LIGHT_VISUAL_*                                                                  */
    float fc_weight;
    int eval;                          /* as nerftex_curved_light_infer_desc                                                      */
    float* sigma;                      /* [B] fp32                                                                                */
    float* rgbs;                       /* [B,3] fp32                                                                              */
    float* shading_normal;             /* [B,3] fp32 or NULL (not written)                                                        */
    const int32_t* units_dev;
    uint32_t rows_per_unit;
    void* scratch;                     /* caller-owned, 256-byte aligned, >= nerftex_curved_light_patch_infer_scratch_bytes(B)    */
    size_t scratch_bytes;
} nerftex_curved_light_patch_infer_desc;
size_t nerftex_curved_light_patch_infer_scratch_bytes(uint32_t B);
int nerftex_curved_light_patch_infer(const nerftex_curved_light_patch_infer_desc* d, void* stream);

/* -------------------------------------------------------------------------
 * Extension: relighting through the four lit chains above -- one imported lighting per visibility probe (the reference's shade_visibility, its
 * default under an imported environment map) and its `euler` lighting rotation (network_curvedfield.py:303-308).  Each _relit entry is its
 * chain's entry with a second, optional descriptor; the chain's own descriptor, scratch query, launches in front of the closing kernel and rows
 * contract are unchanged.  r == NULL, or K == 0 with a NULL rotation: the chain's entry itself, the same launches, the same bits (the plain
 * entries are this case).  Otherwise the closing launch is a second kernel that, per unmarked live row inside the mask,
 *   normalises the raw coarse normal the back half holds twice as n / (|n| + 1e-5) in fp32 (tools/map.py:720, network_curvedfield.py:295),
 *   rotation: rotates the view direction, the shading normal the light mid wrote and that coarse normal by the 3 x 3 matrix -- einsum('ab,nb->na')
 *             under fp16 autocast: matrix and vector rounded to half, the three products added in fp32 in ascending b, the sum rounded to half,
 *   K > 0:    picks the probe as nerftex_sh_light_probe_forward does ((x px + y py) + z pz in fp32 on the (rotated) coarse normal, the lowest
 *             index among equal maxima) and shades with that probe's table; d->env_shs is then not read for shading,
 *   shades with the row function of nerftex_sh_light_forward.
 * shading_normal, where asked for, stays what the light mid wrote: the UNROTATED shading normal.  rotation is read on the device when the kernel
 * runs: new values in the same buffer need no new call sequence (a captured call replays with them).  Nothing is allocated; capturable.
 * NERFTEX_ERR_INVALID with a message, before anything is launched, behind the chain's own shape refusals and in front of its B == 0 return:
 * K > 256 (the probe kernel's limit); K > 0 with a NULL probes or probe_shs; K > 0 with n_color != 3; a non-NULL r with eval == 0 (imported
 * lighting and the rotation are eval-only, as in the reference); a rotation that is not 4-byte aligned.
 * ------------------------------------------------------------------------- */
typedef struct nerftex_relight_desc { /* device pointers */
    const float* probes;               /* [K,3] fp32 probe directions, or NULL with K == 0                                        */
    const float* probe_shs;            /* [K,9,3] fp32: one lighting per probe                                                    */
    uint32_t K;                        /* 0: no probes (the chain descriptor's env_shs lights every row)                          */
    const float* rotation;             /* [9] fp32 row-major, 4-byte aligned, or NULL: no rotation                                */
} nerftex_relight_desc;
int nerftex_curved_light_infer_relit(const nerftex_curved_light_infer_desc* d, const nerftex_relight_desc* r, void* stream);
int nerftex_curved_light_import_infer_relit(const nerftex_curved_light_import_infer_desc* d, const nerftex_relight_desc* r, void* stream);
int nerftex_curved_light_shape_infer_relit(const nerftex_curved_light_shape_infer_desc* d, const nerftex_relight_desc* r, void* stream);
int nerftex_curved_light_patch_infer_relit(const nerftex_curved_light_patch_infer_desc* d, const nerftex_relight_desc* r, void* stream);

/* -------------------------------------------------------------------------
 * Extension: the SH light head of the curved field -- SH_EnvmapMaterialNet.forward behind its BRDF MLP (nerf/sh_light_model.py:554-616) -- as one
 * streaming kernel per direction instead of ~40 framework ops per sample batch, the framework's arithmetic at its rounding points:
 *   albedo = half(sigmoid(brdf[:, :3])), spec_w = half(sigmoid(brdf[:, 3]))              (fp32 sigmoid narrowed to half)
 *   diffuse  = albedo * clamp0(sum_{k<9} env_shs[k] lobe[k] Y_k(n))                      (svox2 basis; lobe = [3.14, 2.09 x 3, 0.79 x 5] / pi)
 *   specular = spec_w * sum_{k<9} env_shs[k] lobe[k] Y_k(w),  w = normalize(2 cos n + r), r = d / (|d| + 1e-9), cos = -(r . n)   (SPECULAR flag;
 *              the glossiness brdf[:, 4] does not enter: the reference's band attenuation is exp(0) as executed)
 *   color    = safe_pow(clamp0(diffuse + specular), 1 / gamma);  specular / diffuse out = safe_pow(clamp01(.), 1 / gamma);  albedo out = clamp01(albedo)
 * all fp32 behind the sigmoids, every operation rounded on its own.  Rows with mask[b] == 0 give 0 in every output and receive a zero grad_brdf row.
 * nerftex_sh_light_backward recomputes the forward from the inputs (nothing saved) and writes
 *   grad_brdf    [B, brdf_stride] fp16: columns 0..3 through the fp16 sigmoid backward (half(g) (1 - y)) y, columns 4.. zero
 *   grad_env_shs [n_sh, n_color] fp32, OVERWRITTEN: rows 0..8 the sum over B -- wave sums, workgroup partials in `scratch`, a closing launch that adds
 *                them in an order fixed by B alone: the same bits on every run -- rows 9.. zero.
 * B == 0: NERFTEX_OK; the backward still writes grad_env_shs = 0.  NERFTEX_ERR_INVALID with a message, before anything is launched: a NULL descriptor
 * or a NULL buffer that the call needs, n_sh < 9, n_color other than 1 or 3, brdf_stride < 5, gamma not positive and finite, an unknown flag, a
 * scratch smaller than nerftex_sh_light_scratch_bytes(B).  Nothing is allocated and the host never waits: both calls can be captured.
 * ------------------------------------------------------------------------- */
#define NERFTEX_SH_LIGHT_SPECULAR 1
typedef struct nerftex_sh_light_desc { /* device pointers unless noted */
    const void* brdf;                  /* [B, brdf_stride] fp16, columns 0..4 used (stride 16 from the BRDF MLP)                  */
    uint32_t brdf_stride;
    const float* normals;              /* [B,3] fp32 shading normals, already normalised                                          */
    const float* dirs;                 /* [B,3] fp32 view directions                                                              */
    const float* env_shs;              /* [n_sh, n_color] fp32; n_sh >= 9; n_color 1 (white light) or 3                           */
    uint32_t n_sh, n_color;
    const uint8_t* mask;               /* [B] bytes or NULL: rows with 0 give 0 and receive 0                                     */
    uint32_t B;
    float gamma;                       /* host value                                                                              */
    uint32_t flags;                    /* NERFTEX_SH_LIGHT_SPECULAR                                                               */
    float* color;                      /* [B,3] fp32                                                                              */
    float* specular;                   /* [B,3] fp32 or NULL                                                                      */
    float* diffuse;                    /* [B,3] fp32 or NULL                                                                      */
    float* albedo;                     /* [B,3] fp32 or NULL                                                                      */
    const float* grad_color;           /* backward: [B,3] fp32 in                                                                 */
    void* grad_brdf;                   /* backward: [B, brdf_stride] fp16 out                                                     */
    float* grad_env_shs;               /* backward: [n_sh, n_color] fp32 out                                                      */
    void* scratch;                     /* backward: caller-owned, >= nerftex_sh_light_scratch_bytes(B) bytes                      */
    size_t scratch_bytes;
} nerftex_sh_light_desc;
int nerftex_sh_light_forward(const nerftex_sh_light_desc* d, void* stream);
int nerftex_sh_light_backward(const nerftex_sh_light_desc* d, void* stream);
size_t nerftex_sh_light_scratch_bytes(uint32_t B);

/* -------------------------------------------------------------------------
 * Extension: the head under imported lighting with visibility (sh_light_model.py:561-571, eval with import_envmap and shade_visibility): every
 * row is lit by one of K coefficient sets, the one whose probe direction is closest to the row's secondary (coarse) normal n2:
 *   k* = argmax_k (n2 . probes[k]),  the dot product (x px + y py) + z pz in fp32, every operation rounded on its own; the LOWEST index among
 *        equal maxima
 *   the row is then shaded exactly as nerftex_sh_light_forward shades it with n_color = 3 and env_shs = probe_shs[k*]  ([9,3])
 * A workgroup stages probes and probe_shs (x lobe) in LDS once, K * 120 bytes.  Rows with mask[b] == 0 give 0 in every output.  Forward only: the
 * reference uses imported lighting only when not training.  B == 0: NERFTEX_OK.  NERFTEX_ERR_INVALID with a message, before anything is
 * launched: a NULL descriptor or a NULL buffer that the call needs, K == 0 or K > 256, brdf_stride < 5, gamma not positive and finite, an unknown
 * flag.  Nothing is allocated and the host never waits: the call can be captured.
 * ------------------------------------------------------------------------- */
typedef struct nerftex_sh_light_probe_desc { /* device pointers unless noted */
    const void* brdf;                  /* [B, brdf_stride] fp16, columns 0..4 used, as nerftex_sh_light_desc                      */
    uint32_t brdf_stride;
    const float* normals;              /* [B,3] fp32 shading normals, already normalised                                          */
    const float* dirs;                 /* [B,3] fp32 view directions                                                              */
    const float* normals_secondary;    /* [B,3] fp32: what the probe is chosen by                                                 */
    const float* probes;               /* [K,3] fp32 probe directions                                                             */
    const float* probe_shs;            /* [K,9,3] fp32: one lighting per probe                                                    */
    uint32_t K;                        /* 1 .. 256                                                                                */
    const uint8_t* mask;               /* [B] bytes or NULL: rows with 0 give 0                                                   */
    uint32_t B;
    float gamma;                       /* host value                                                                              */
    uint32_t flags;                    /* NERFTEX_SH_LIGHT_SPECULAR                                                               */
    float* color;                      /* [B,3] fp32                                                                              */
    float* specular;                   /* [B,3] fp32 or NULL                                                                      */
    float* diffuse;                    /* [B,3] fp32 or NULL                                                                      */
    float* albedo;                     /* [B,3] fp32 or NULL                                                                      */
} nerftex_sh_light_probe_desc;
int nerftex_sh_light_probe_forward(const nerftex_sh_light_probe_desc* d, void* stream);

/* -------------------------------------------------------------------------
 * Extension: SH lighting fitted to an equirectangular environment map -- EnvMap2SH (nerf/sh_light_model.py:730-766): up to max_steps iterations
 * of torch.optim.Adam(lr) on  loss(c) = mean((SH2Envmap(c) - envmap)^2)  from c = 0.  The objective is linear least squares in the 27 numbers
 * c[0..8][0..2], so the map is read once:
 *   moments    one thread per pixel (grid-stride above 262 144 pixels): direction (cos theta sin phi, cos phi, sin theta sin phi) in fp32, the
 *              nine svox2 bases Y in fp32, then in fp64  G = sum Y Y^T (45 entries), b = sum Y y^T (27), s = sum y^2 (3): wave butterfly, the four
 *              waves in order through LDS, one partial per workgroup in `scratch`; the grid is a function of H W alone
 *   iteration  ONE wave: sums the partials in workgroup order, then runs the loop, lane k * 3 + c owning c[k][c]:
 *              loss_t = (c^T G c - 2 c^T b + s) / (3 H W) in fp64 of the parameters BEFORE the update; g = fp32(2 / (3 H W) (G c - b));
 *              torch's single-tensor Adam on fp32 state (betas 0.9 / 0.999, eps 1e-8, step size lr / (1 - 0.9^t) and sqrt(1 - 0.999^t)
 *              from double, rounded to fp32):  m += 0.1 (g - m);  v = 0.999 v + (0.001 g) g;  c += (-step_size m) / (sqrt(v) / bc2 + eps)
 *              and stops AFTER the update of the first step t (counted from 1) with loss_t < min_loss and t - 1 > min_steps, or after max_steps.
 * env_shs rows 9.. are written as 0 (they receive no gradient in the reference).  steps_run = the number of updates made; final_loss = the last
 * loss_t.  Two launches, nothing allocated, the host never waits: the call can be captured; the same bits on every run.
 * NERFTEX_ERR_INVALID with a message, before anything is launched: a NULL descriptor or buffer, H W == 0, n_sh < 9, lr not positive and finite,
 * max_steps == 0, scratch or final_loss not 8-byte aligned, scratch smaller than nerftex_envmap_fit_scratch_bytes(H, W).
 * ------------------------------------------------------------------------- */
typedef struct nerftex_envmap_fit_desc { /* device pointers unless noted */
    const float* envmap;               /* [H,W,3] fp32                                                                            */
    const float* phi;                  /* [H] fp32 polar angles: torch.linspace(0, pi, H)                                         */
    const float* theta;                /* [W] fp32 azimuths: torch.linspace(-pi / 2, 3 pi / 2, W)                                 */
    uint32_t H, W;
    uint32_t n_sh;                     /* rows of env_shs, >= 9                                                                   */
    uint32_t max_steps;                /* the reference: 5000                                                                     */
    uint32_t min_steps;                /* the reference: 2000                                                                     */
    double lr;                         /* host value; the reference: 1e-2                                                         */
    double min_loss;                   /* host value; the reference: 1e-5                                                         */
    float* env_shs;                    /* [n_sh,3] fp32 out                                                                       */
    int32_t* steps_run;                /* [1] out                                                                                 */
    double* final_loss;                /* [1] out                                                                                 */
    void* scratch;                     /* caller-owned, 8-byte aligned, >= nerftex_envmap_fit_scratch_bytes(H, W) bytes           */
    size_t scratch_bytes;
} nerftex_envmap_fit_desc;
int nerftex_envmap_fit(const nerftex_envmap_fit_desc* d, void* stream);
size_t nerftex_envmap_fit_scratch_bytes(uint32_t H, uint32_t W);

/* -------------------------------------------------------------------------
 * Extension: the per-probe visibility lighting of an imported map -- load_envmap_with_visibility without a file (nerf/sh_light_model.py:653-665)
 * around fit_product_of_SHs (:692-709).  For each probe p of K, from sh = env_shs[:9], `rounds` steps of torch.optim.Adam(lr) on
 *   loss(sh) = mean over `batch` sphere points x of  sum_c ( Y(x) . sh[:, c] - (Y(x) . env_shs[:9, c]) (Y(x) . lobes[p]) )^2
 * with Y the nine svox2 bases (the polynomials and signs of nerf/spherical_harmonics.py, degree 2) and fresh points every step.  AS THE REFERENCE
 * EXECUTES IT: it never clears the gradient, so the gradient Adam sees at step t is the SUM of the gradients of steps 1..t.  The result is not
 * converged; it is defined by this trajectory and by the points.
 *   points     given ([K, rounds, batch, 3]): read.  NULL: point (p, r, i) comes from a counter hash keyed by (seed, p, r, i) -- two uniforms in
 *              [0, 1) with 24 bits, phi = 2 pi u1, theta = acos(1 - 2 u2), (cos phi sin theta, sin phi sin theta, cos theta), the reference's
 *              expression -- so the result does not depend on the launch shape.  THIS LIBRARY'S OWN STREAM, NOT torch.rand's: a run with its own
 *              points agrees with the reference's only statistically.  points_out, if given, receives every point used.
 *   a round    one workgroup of 256 threads per probe walks all rounds; thread t takes points t, t + 256, ...: per point the nine bases, the
 *              three residuals 2 (pred - gt) / batch, 27 partial sums; the wave's sum on the DPP paths, the four waves in order through LDS;
 *              added to the running gradient; torch's single-tensor Adam on fp32 state (betas 0.9 / 0.999, eps 1e-8, step size lr / (1 - 0.9^t)
 *              and sqrt(1 - 0.999^t) from double, rounded to fp32):  m += 0.1 (g - m);  v = 0.999 v + (0.001 g) g;
 *              sh += (-step_size m) / (sqrt(v) / bc2 + eps).  All fp32, every operation rounded on its own, the order of every sum fixed.
 * One launch, nothing allocated, the host never waits: the call can be captured; the same bits on every run.
 * NERFTEX_ERR_INVALID with a message, before anything is launched: a NULL descriptor, env_shs, lobes or tables, n_sh < 9, K == 0 or K > 256,
 * rounds == 0 or batch == 0, lr not positive and finite.
 * ------------------------------------------------------------------------- */
typedef struct nerftex_envmap_vis_fit_desc { /* device pointers unless noted */
    const float* env_shs;              /* [n_sh,3] fp32: the imported lighting; rows 0..8 are read                                */
    uint32_t n_sh;                     /* rows of env_shs, >= 9                                                                   */
    const float* lobes;                /* [K,9] fp32: the visibility lobe rotated onto each probe; one lobe for all three colours */
    uint32_t K;                        /* 1 .. 256                                                                                */
    uint32_t rounds;                   /* the reference: 800                                                                      */
    uint32_t batch;                    /* points per round; the reference: 1024.  Any positive number                             */
    double lr;                         /* host value; the reference: 1e-3                                                         */
    uint64_t seed;                     /* host value; keys the points when `points` is NULL                                       */
    const float* points;               /* [K,rounds,batch,3] fp32 or NULL                                                         */
    float* points_out;                 /* [K,rounds,batch,3] fp32 or NULL                                                         */
    float* tables;                     /* [K,9,3] fp32 out                                                                        */
} nerftex_envmap_vis_fit_desc;
int nerftex_envmap_vis_fit(const nerftex_envmap_vis_fit_desc* d, void* stream);

/* grad_hc [B,16] fp16 = sigmoid backward of the fp16-narrowed grad_rgbs, columns 3..15 zero                      */
int nerftex_field_out_backward(const float* grad_rgbs, const float* rgbs, uint32_t B, void* grad_hc, void* stream);

/* -------------------------------------------------------------------------
 * train step ends (harness-level, not reference entry points: the reference leaves both to torch ops)
 * ------------------------------------------------------------------------- */

/* Tail of the training render + loss (nerf/renderer.py:417-425, MSE of nerf/utils.py:602-640), all fp32:
 *   image_out [N,3] = image + (1 - weights_sum) * bg;   depth_out [N] = clamp(depth - nears, 0) / (fars - nears);
 *   *loss = mean((image_out - target)^2) * loss_mul     (block partials added in index order: run-to-run identical).
 * partial: >= ceil(N/256) floats of scratch; ticket: one uint32 that is 0 on entry and left 0.                       */
int nerftex_render_tail_forward(const float* weights_sum, const float* depth, const float* image, const float* nears,
                                const float* fars, const float* target, float bg, float loss_mul, uint32_t N,
                                float* image_out, float* depth_out, float* partial, uint32_t* ticket, float* loss,
                                const float* scale, float* scaled_loss, void* stream);
/* scale (device float of a loss scaler, or NULL) / scaled_loss (or NULL): *scaled_loss = *loss * *scale, what
 * GradScaler.scale(loss) would compute; the backward below then takes the same scale.
 * grad_image [N,3] = (2 / 3N) * (image_out - target) * (*grad_loss * *scale * loss_mul);  grad_weights_sum [N] = -sum_c(grad_image) * bg */
int nerftex_render_tail_backward(const float* grad_loss, const float* scale, float loss_mul, const float* image_out,
                                 const float* target, float bg, uint32_t N, float* grad_image, float* grad_weights_sum,
                                 void* stream);

/* nerftex_render_tail_backward followed by nerftex_composite_rays_train_backward as ONE launch: the wave that walks a ray backwards
 * first forms its grad_image / grad_weights_sum from image_out, target and the loss gradient (never stored).  Same gradients, bit for
 * bit.  (image_out: what nerftex_render_tail_forward wrote; weights_sum, image: what nerftex_composite_rays_train_forward wrote.) */
int nerftex_composite_tail_backward(const float* grad_loss, const float* scale, float loss_mul, const float* image_out,
                                    const float* target, float bg, const float* sigmas, const float* rgbs, const float* deltas,
                                    const int32_t* rays, const float* weights_sum, const float* image, uint32_t M, uint32_t N,
                                    float* grad_sigmas, float* grad_rgbs, void* stream);

/* Extension (round 6): the two launches above with the STEP FLAGS of the dead-sample skip.  nerftex_render_tail_forward_live also clears
 * step_live[0 .. n_steps) (n_steps = ceil(M / 32) words; rides on a launch the step has anyway); nerftex_composite_tail_backward_live sets the word
 * of every 32-sample step that holds a sample whose grad_sigma or grad_rgb is not exactly zero (ballot + one leader lane per step; nan / inf count
 * as non-zero).  step_live NULL = the plain calls.                                                                                        */
int nerftex_render_tail_forward_live(const float* weights_sum, const float* depth, const float* image, const float* nears, const float* fars,
                                     const float* target, float bg, float loss_mul, uint32_t N, float* image_out, float* depth_out, float* partial,
                                     uint32_t* ticket, float* loss, const float* scale, float* scaled_loss, uint32_t* step_live, uint32_t n_steps,
                                     void* stream);
int nerftex_composite_tail_backward_live(const float* grad_loss, const float* scale, float loss_mul, const float* image_out, const float* target,
                                         float bg, const float* sigmas, const float* rgbs, const float* deltas, const int32_t* rays,
                                         const float* weights_sum, const float* image, uint32_t M, uint32_t N, float* grad_sigmas, float* grad_rgbs,
                                         uint32_t* step_live, void* stream);

/* Extension (round 6): the compositing of a TRAINING STEP as one launch -- nerftex_composite_rays_train_forward, nerftex_render_tail_forward and
 * nerftex_composite_tail_backward (raymarching.cu:739-767 + :843-880 with nerf/renderer.py:417-425 and the MSE between them): the wave that walks a
 * ray forward keeps what the backward walk needs in registers, forms the blend, the depth normalisation, the squared error and the loss gradient
 * when the ray's sums are complete, and writes grad_sigmas / grad_rgbs.  All outputs of the three calls, bit for bit: weights_sum, depth [N],
 * image [N,3] (raw), image_out [N,3], depth_out [N], loss and scaled_loss (= loss * *scale; scale NULL: = loss) [1], and grad_sigmas [M],
 * grad_rgbs [M,3] = the gradient of scaled_loss for a ROOT GRADIENT OF ONE (any other: nerftex_composite_tail_backward with the outputs of this
 * call).  The gradient buffers need not be zero-filled (as for nerftex_composite_tail_backward: this library's ordered ray records).  err [N]:
 * scratch (the rays' squared errors; a second, one-workgroup launch adds them in nerftex_render_tail_forward's order).  step_live: NULL or
 * ceil(M / 32) words that are ZERO ON ENTRY -- set as nerftex_composite_tail_backward_live sets them; nerftex_field_backward_live_consume
 * zeroes them again.  loss NULL: the second launch is not made (err[] goes to nerftex_field_backward_live_consume's nerftex_step_loss).
 * N <= 262144, N > 0, M > 0.                                                                                          */
int nerftex_composite_step(const float* sigmas, const float* rgbs, const float* deltas, const int32_t* rays, uint32_t M, uint32_t N,
                           const float* nears, const float* fars, const float* target, float bg, float loss_mul, const float* scale,
                           float* weights_sum, float* depth, float* image, float* image_out, float* depth_out, float* err, float* loss,
                           float* scaled_loss, float* grad_sigmas, float* grad_rgbs, uint32_t* step_live, void* stream);

/* The criterion of a training step, its per-ray loss and the error map (nerf/utils.py:617-632, --error_map): the three train-step ends above
 * trained one objective, the mean squared error.  The reference's NeRF-Texture trainer uses torch.nn.L1Loss (main.py:187), its ngp trainer
 * MSELoss with a Huber loss beside it (main_nerf.py:104-106).  With a nerftex_step_loss_desc the same launches form
 *   element e(d), d = image_out - target:  MSE d^2;  L1 |d|;  HUBER 0.5 d^2 where |d| <= delta, else delta (|d| - 0.5 delta)   (torch's)
 *   *loss = sum(e) / 3N * loss_mul;   grad_image = (de/dd) * g / 3N  (L1: sign(d), 0 at d == 0;  HUBER: d where |d| <= delta, else delta sign(d))
 *   ray_loss[n] = (sum over the ray's three channels of e) / 3: the reference's criterion(pred, gt).mean(-1), before loss_mul and scale;
 *   error_map[i] = keep * error_map[i] + take * ray_loss[n] for i = error_inds[n] when 0 <= i < error_cells; any other index -- negative
 *   ones included -- touches nothing.  A plain read-modify-write by the thread that holds the ray's error, no extra launch: the indices of one
 *   call are distinct (torch.multinomial without replacement); with duplicates ONE of the candidates lands, as with torch's scatter_.  The map
 *   is written by the forward, whether or not a loss scaler later skips the step (the reference writes it before backward() too).
 * An unknown kind, a Huber delta that is not finite and > 0, or a map without indices (or indices without a map): NERFTEX_ERR_INVALID,
 * nothing is launched.  desc NULL: the call is the entry it extends.                                                                     */
#define NERFTEX_LOSS_MSE 0
#define NERFTEX_LOSS_L1 1
#define NERFTEX_LOSS_HUBER 2
typedef struct nerftex_step_loss_desc {
    uint32_t kind;             /* NERFTEX_LOSS_MSE / _L1 / _HUBER */
    float param;               /* Huber delta (> 0); ignored otherwise */
    float* ray_loss;           /* [N] or NULL */
    float* error_map;          /* [error_cells] or NULL */
    const int64_t* error_inds; /* [N]; required iff error_map */
    uint64_t error_cells;
    float keep, take;          /* the reference's 0.1f, 0.9f */
} nerftex_step_loss_desc;
/* nerftex_render_tail_forward_live / nerftex_render_tail_backward / nerftex_composite_tail_backward_live / nerftex_composite_step with a
 * descriptor: the criterion's loss instead of the squared error, everything else as documented there (err [N] of nerftex_composite_step_ex: the
 * rays' summed elements -- nerftex_step_loss finishes the loss of any criterion).  The two backward entries read kind and param only.       */
int nerftex_render_tail_forward_ex(const float* weights_sum, const float* depth, const float* image, const float* nears, const float* fars,
                                   const float* target, float bg, float loss_mul, uint32_t N, float* image_out, float* depth_out, float* partial,
                                   uint32_t* ticket, float* loss, const float* scale, float* scaled_loss, uint32_t* step_live, uint32_t n_steps,
                                   const nerftex_step_loss_desc* desc, void* stream);
int nerftex_render_tail_backward_ex(const float* grad_loss, const float* scale, float loss_mul, const float* image_out, const float* target,
                                    float bg, uint32_t N, float* grad_image, float* grad_weights_sum, const nerftex_step_loss_desc* desc,
                                    void* stream);
int nerftex_composite_tail_backward_ex(const float* grad_loss, const float* scale, float loss_mul, const float* image_out, const float* target,
                                       float bg, const float* sigmas, const float* rgbs, const float* deltas, const int32_t* rays,
                                       const float* weights_sum, const float* image, uint32_t M, uint32_t N, float* grad_sigmas, float* grad_rgbs,
                                       uint32_t* step_live, const nerftex_step_loss_desc* desc, void* stream);
int nerftex_composite_step_ex(const float* sigmas, const float* rgbs, const float* deltas, const int32_t* rays, uint32_t M, uint32_t N,
                              const float* nears, const float* fars, const float* target, float bg, float loss_mul, const float* scale,
                              float* weights_sum, float* depth, float* image, float* image_out, float* depth_out, float* err, float* loss,
                              float* scaled_loss, float* grad_sigmas, float* grad_rgbs, uint32_t* step_live, const nerftex_step_loss_desc* desc,
                              void* stream);

/* A background per ray and RGBA pixels: what the reference's train_step does for every image with an alpha channel (nerf/utils.py:602-615)
 *   bg_color = torch.rand_like(images[..., :3]);  gt_rgb = images[..., :3] * images[..., 3:] + bg_color * (1 - images[..., 3:])
 * and renderer.py:424 blends image + (1 - weights_sum)[:, None] * bg_color.  The four _px entries are the _ex entries with a second descriptor;
 * the scalar `bg` argument is then ignored.  fp32, every operation rounded on its own, in the order of the torch expressions:
 *   target     gt[c] = rgba[c] * a + bg[c] * (1 - a),  a = rgba[3]   -- written to target_out by the two forwards (nerftex_render_tail_forward_px,
 *              nerftex_composite_step_px, which also keeps it in registers); the two backwards read target_out as their target
 *   blend      image_out[c] = image[c] + (1 - weights_sum) * bg[c]
 *   criterion, ray_loss, error map, loss, scaled loss: unchanged, on d = image_out - gt
 *   opacity    sum = 0; sum += gi0 * bg[0]; sum += gi1 * bg[1]; sum += gi2 * bg[2]; grad_weights_sum = -sum   (bg == 1: the scalar form's bits)
 * Without rgba the entry's `target` [N,3] is the target, as in the _ex entries.  The step flags, the deferred loss (nerftex_step_loss) and the
 * trailer see err[] and the gradients only: they work with these entries as with _ex.
 * NOT produced: a gradient with respect to the background or to alpha.  Out of scope: the background network (bg_radius > 0), whose colours
 * would need that gradient, and color_space == 'linear'.
 * NERFTEX_ERR_INVALID, nothing launched: bg_rays NULL; rgba and target both given, or neither; rgba without target_out.
 * pixels NULL: the call is the _ex entry it extends -- the same launch, the same bits.                                                      */
typedef struct nerftex_step_pixels_desc {
    const float* bg_rays; /* [N,3] per-ray background; required */
    const float* rgba;    /* [N,4] or NULL; non-NULL: the target is formed from it and `target` must be NULL */
    float* target_out;    /* [N,3]; required iff rgba: the blended gt_rgb, written by the forward */
} nerftex_step_pixels_desc;
int nerftex_render_tail_forward_px(const float* weights_sum, const float* depth, const float* image, const float* nears, const float* fars,
                                   const float* target, float bg, float loss_mul, uint32_t N, float* image_out, float* depth_out, float* partial,
                                   uint32_t* ticket, float* loss, const float* scale, float* scaled_loss, uint32_t* step_live, uint32_t n_steps,
                                   const nerftex_step_loss_desc* desc, const nerftex_step_pixels_desc* pixels, void* stream);
int nerftex_render_tail_backward_px(const float* grad_loss, const float* scale, float loss_mul, const float* image_out, const float* target,
                                    float bg, uint32_t N, float* grad_image, float* grad_weights_sum, const nerftex_step_loss_desc* desc,
                                    const nerftex_step_pixels_desc* pixels, void* stream);
int nerftex_composite_tail_backward_px(const float* grad_loss, const float* scale, float loss_mul, const float* image_out, const float* target,
                                       float bg, const float* sigmas, const float* rgbs, const float* deltas, const int32_t* rays,
                                       const float* weights_sum, const float* image, uint32_t M, uint32_t N, float* grad_sigmas, float* grad_rgbs,
                                       uint32_t* step_live, const nerftex_step_loss_desc* desc, const nerftex_step_pixels_desc* pixels,
                                       void* stream);
int nerftex_composite_step_px(const float* sigmas, const float* rgbs, const float* deltas, const int32_t* rays, uint32_t M, uint32_t N,
                              const float* nears, const float* fars, const float* target, float bg, float loss_mul, const float* scale,
                              float* weights_sum, float* depth, float* image, float* image_out, float* depth_out, float* err, float* loss,
                              float* scaled_loss, float* grad_sigmas, float* grad_rgbs, uint32_t* step_live, const nerftex_step_loss_desc* desc,
                              const nerftex_step_pixels_desc* pixels, void* stream);

/* One Adam step (main_nerf.py:128: betas (0.9, 0.99), eps 1e-15, no weight decay) of an fp32 master table from the
 * fp16 gradient the encoder backward produced, writing the fp16 copy the next forward reads: param, exp_avg,
 * exp_avg_sq [n] fp32 in place, grad_half [n] fp16 in, param_half [n] fp16 out.  step: device float, already
 * incremented (1 on the first step).  grad_scale / found_inf: device floats of a GradScaler or NULL -- the gradient
 * is divided by *grad_scale; the whole step is skipped when *found_inf == 1.  Arithmetic as torch's fused Adam.    */
int nerftex_table_adam_step(float* param, float* exp_avg, float* exp_avg_sq, const void* grad_half, void* param_half,
                            uint64_t n, const float* step, double lr, double beta1, double beta2, double eps,
                            const float* grad_scale, const float* found_inf, void* stream);
/* The same for up to 8 tensors in one launch (host arrays of device pointers / lengths); the step number used is
 * *step + step_offset.                                                                                            */
int nerftex_adam_half_step(int count, float* const* params, float* const* exp_avgs, float* const* exp_avg_sqs,
                           const void* const* grads_half, void* const* params_half, const uint64_t* n, const float* step,
                           float step_offset, double lr, double beta1, double beta2, double eps, const float* grad_scale,
                           const float* found_inf, void* stream);
/* Device side of torch.amp.GradScaler for fp16 gradients.  check: *found_inf = 1 if any element of up to 8 fp16 tensors
 * is inf / nan (never cleared here).  update (amp_update_scale_): found_inf != 0 -> scale *= backoff_factor, tracker = 0;
 * else tracker += 1, at growth_interval scale *= growth_factor (if finite) and tracker = 0, and *step += 1 (step may be
 * NULL); found_inf is cleared for the next step.                                                                   */
int nerftex_amp_check_half(int count, const void* const* grads_half, const uint64_t* n, float* found_inf, void* stream);
/* nerftex_adam_half_step (step number *step + 1, gradients divided by *scale, skipped when *found_inf == 1) followed, in the same
 * launch, by nerftex_amp_update on the same scale / found_inf / step words: the block that finishes last does it (ticket: one
 * uint32 that is 0 on entry and left 0).                                                                                  */
int nerftex_adam_half_step_amp(int count, float* const* params, float* const* exp_avgs, float* const* exp_avg_sqs,
                               const void* const* grads_half, void* const* params_half, const uint64_t* n, float* step,
                               double lr, double beta1, double beta2, double eps, float* scale, int32_t* growth_tracker,
                               float* found_inf, uint32_t* ticket, double growth_factor, double backoff_factor,
                               int growth_interval, void* stream);
/* Extension (round 5): the three calls above with a 16-bit type PER TENSOR -- bit t of bf16_mask set: tensor t's gradient and its narrowed
 * copy are bf16 (round to nearest even, as tensor.to(torch.bfloat16)), clear: fp16.  A bf16 field (BASELINE configs[2]) keeps its hash table
 * and the table's gradient in fp16 (gridencoder/grid.py:38-41 casts the table to half under ANY autocast) and its MLP weights in bf16: one
 * launch updates all of them.  bf16_mask 0 == the _half forms.                                                                        */
int nerftex_adam_mixed_step(int count, float* const* params, float* const* exp_avgs, float* const* exp_avg_sqs,
                            const void* const* grads16, void* const* params16, const uint64_t* n, uint32_t bf16_mask, const float* step,
                            float step_offset, double lr, double beta1, double beta2, double eps, const float* grad_scale,
                            const float* found_inf, void* stream);
int nerftex_adam_mixed_step_amp(int count, float* const* params, float* const* exp_avgs, float* const* exp_avg_sqs,
                                const void* const* grads16, void* const* params16, const uint64_t* n, uint32_t bf16_mask, float* step,
                                double lr, double beta1, double beta2, double eps, float* scale, int32_t* growth_tracker, float* found_inf,
                                uint32_t* ticket, double growth_factor, double backoff_factor, int growth_interval, void* stream);
/* Extension (round 6): nerftex_adam_mixed_step_amp over DOUBLE-BUFFERED state -- the end of a step whose hashed table rows
 * nerftex_grid_encode_backward_adam has already updated.  Reads set [*live & 1] (params / exp_avgs / exp_avg_sqs = set 0, the *1 arrays = set 1),
 * writes the other one; the loss scaler's update (last block, as in the _amp forms) flips *live iff the step is applied.  On a skipped step the
 * repair range -- repair_n 16-bit elements at repair_half, the fp32 elements they narrow at repair_param0 / repair_param1 -- is re-derived from
 * the live set (repair_n 0: none).                                                                                                        */
int nerftex_adam_mixed_step_amp_db(int count, float* const* params, float* const* exp_avgs, float* const* exp_avg_sqs, float* const* params1,
                                   float* const* exp_avgs1, float* const* exp_avg_sqs1, const void* const* grads16, void* const* params16,
                                   const uint64_t* n, uint32_t bf16_mask, float* step, double lr, double beta1, double beta2, double eps,
                                   float* scale, int32_t* growth_tracker, float* found_inf, uint32_t* ticket, double growth_factor,
                                   double backoff_factor, int growth_interval, uint32_t* live, void* repair_half, const float* repair_param0,
                                   const float* repair_param1, uint64_t repair_n, void* stream);
/* Extension: nerftex_adam_mixed_step_amp and nerftex_adam_mixed_step_amp_db with the learning rate of the step taken from a schedule
 * (nerftex_lr_schedule, above): base_lr * factor[min(*iter, n - 1)] in place of lr, and the loss scaler's tail also advances *iter -- on a
 * skipped step as well (*step, Adam's bias-correction count, still advances on applied steps only).  Same bits as the unscheduled calls fed that
 * product as lr.                                                                                                                              */
int nerftex_adam_mixed_step_amp_sched(int count, float* const* params, float* const* exp_avgs, float* const* exp_avg_sqs,
                                      const void* const* grads16, void* const* params16, const uint64_t* n, uint32_t bf16_mask, float* step,
                                      double base_lr, const nerftex_lr_schedule* sched, double beta1, double beta2, double eps, float* scale,
                                      int32_t* growth_tracker, float* found_inf, uint32_t* ticket, double growth_factor, double backoff_factor,
                                      int growth_interval, void* stream);
int nerftex_adam_mixed_step_amp_db_sched(int count, float* const* params, float* const* exp_avgs, float* const* exp_avg_sqs, float* const* params1,
                                         float* const* exp_avgs1, float* const* exp_avg_sqs1, const void* const* grads16, void* const* params16,
                                         const uint64_t* n, uint32_t bf16_mask, float* step, double base_lr, const nerftex_lr_schedule* sched,
                                         double beta1, double beta2, double eps, float* scale, int32_t* growth_tracker, float* found_inf,
                                         uint32_t* ticket, double growth_factor, double backoff_factor, int growth_interval, uint32_t* live,
                                         void* repair_half, const float* repair_param0, const float* repair_param1, uint64_t repair_n, void* stream);
/* Extension: the schedule for an optimizer that reads its learning rate from a device tensor (torch.optim.Adam(fused=True) with tensor lr: a
 * float32 it reads at each step).  One thread: lr_out[g][0] = (float)(base_lrs[g] * factor[min(*iter, n - 1)]) for g < groups -- the rounding
 * of LRScheduler's group["lr"].fill_(value) -- then *iter += 1.  Launched in front of the optimizer in every step, skipped ones included.
 * base_lrs / lr_out: host arrays of 1..8 entries (lr_out: device fp32 scalars).                                                            */
int nerftex_lr_schedule_publish(const nerftex_lr_schedule* sched, const double* base_lrs, float* const* lr_out, uint32_t groups, void* stream);
int nerftex_amp_check_mixed(int count, const void* const* grads16, const uint64_t* n, uint32_t bf16_mask, float* found_inf, void* stream);
int nerftex_amp_update(float* scale, int32_t* growth_tracker, float* found_inf, float* step, double growth_factor,
                       double backoff_factor, int growth_interval, void* stream);

/* Extension: an exponential moving average of the parameters, kept on the device by the training step itself (the reference trainer wraps its
 * parameters in torch_ema.ExponentialMovingAverage(decay=0.95) and calls update() after every optimizer step: nerf/utils.py:460-462, :1027-1028).
 * One streaming launch, 12 B per parameter, over `count` fp32 tensors of n[t] elements: torch_ema's update() with use_num_updates=True,
 *     u = *num_updates + 1;  d = min(decay, (1 + u) / (10 + u)) in double;  w = (float)(1.0 - d);
 *     per element  tmp = s - p;  tmp = tmp * w;  s = s - tmp      (three fp32 roundings, no fma: the bits of torch's sub, mul_, sub_)
 * p comes from param1[t] when `live` is given and *live & 1, else from param0[t]: behind the last launch of a double-buffered optimizer step
 * (nerftex_adam_mixed_step_amp_db) the live word names the step's parameters, whether the step was applied (flipped) or skipped (left).
 * Every block reads *num_updates and *live once, at its start; with advance != 0 the block that finishes last stores *num_updates = u (ticket:
 * zero on entry, left zero).  count is 1..8 per call: a model with more tensors makes several calls, advance set on the LAST one only -- they
 * all read the same *num_updates and so behave as one update over their union.  Tensors with n[t] == 0 are skipped.
 * NERFTEX_ERR_INVALID, nothing launched: a NULL descriptor, num_updates, ticket, shadow, param0 or n (or a NULL buffer of a non-empty tensor);
 * decay outside (0, 1); count outside 1..8; live without param1; a buffer that is not 16-byte aligned.                                        */
typedef struct nerftex_ema_desc {
    double decay;          /* the cap, 0 < decay < 1 */
    uint32_t* num_updates; /* device word: updates done so far */
    uint32_t* ticket;      /* device word: zero on entry, left zero */
    const uint32_t* live;  /* NULL, or the double-buffered optimizer's live word */
    int advance;           /* != 0: the launch's last block stores *num_updates + 1 */
} nerftex_ema_desc;
int nerftex_ema_update(const nerftex_ema_desc* desc, int count, float* const* shadow, const float* const* param0,
                       const float* const* param1 /* NULL without live */, const uint64_t* n, void* stream);

/* The planar texture synthesized from exported patches (csrc/synthesis.inc): the path the reference's patch_matching_and_quilting.py runs --
 * patchBasedTextureSynthesis with mode 'Cut', quilt off, coarse_KDtree, rotate off, picked_vertices given (close_patch_check), PARM_truncation 0 --
 * and the closing lines of its __main__ (:485-511).  The canvas is filled cell by cell in raster order: the k = 16 examples whose coarse overlap
 * strips are nearest the canvas's (Euclidean, float64 sums over fp32 block sums), the close-patch filter, k doubled while nothing survives, a
 * weighted draw from one uniform number per cell, a minimum-error boundary cut against the left and then the top neighbour, a masked copy.
 * Examples: the P patches, then their row-flipped copies (mirror_hor), then the column-flipped copies of all of those (mirror_vert); they are read
 * through the flips, never stored.  Canvas, databases and outputs are fp32; a copied pixel is the example's pixel bit for bit, a seam's mean is
 * the correctly rounded float64 mean (its fp32 residual is kept beside the canvas for the cuts and for a second mean in a corner); distances, seam
 * energies and the selection are float64 in a fixed order: the same bits from run to run.
 *   create   validates (NERFTEX_ERR_INVALID with a message, before any device call: a NULL descriptor, out or array; P, S, C of 0; match_dim outside
 *            1..C; overlap_size of 0 or above 256; overlap_size * 2 + patch_size != S; a non-square or too small output (output_h != output_w,
 *            output_h <= overlap_size, a canvas side above 16384); attenuation other than 1 or 3; max_patch_res of 0; mode other than
 *            NERFTEX_SYNTH_CUT; quilt set; more than 2^31 - 1 examples or database entries), then builds the two coarse databases
 *            [examples, overlap * ceil(S / block) * match_dim] fp32, block = max(S / max_patch_res, 1), and allocates canvas, ids, id map, log and
 *            workspaces.  The descriptor's three arrays are device memory and must outlive the handle.
 *   resolve  cells [cell_begin, cell_end) in raster order, at most four launches a cell and no host synchronisation: the coarse query, the distances
 *            (examples x slices of the strip, float64 partial sums), the selection and the cuts (one workgroup), the masked copy.  Cell 0 takes
 *            first_patch uncut.  draws [cells] and forced [cells] (or NULL) are DEVICE arrays indexed by the cell (entry 0 unused); with forced the
 *            placed example is forced[cell] while the one the draw picks is still logged.  NERFTEX_ERR_INVALID: first_patch >= examples, a cell
 *            range outside the canvas or not starting where the last call ended, NULL draws.
 *            A cell whose k would exceed the example set (sklearn raises there) sets a device status; the cells behind it do nothing.
 *   finish   the closing remap -- total_id = the sorted distinct ids of canvas_id, sample_tbn = example_tbn[total_id], sample_tbn_ids = canvas_id
 *            as positions in total_id -- then waits for the stream and reports the status: NERFTEX_ERR_EXHAUSTED (with the cell in the message)
 *            if a cell ran out of examples, NERFTEX_ERR_INVALID for a forced id outside the example set or non-finite distances.
 *   result   pointers and sizes (device memory owned by the handle; n_total is valid after finish);  read: an asynchronous device-to-device copy
 *            of one of the arrays, `bytes` being its exact size.
 * The log, per cell: log_ids [cells, NERFTEX_SYNTH_LOG_STRIDE] int32 = k used, survivor count, the id the draw picked, the placed id, the first 16
 * ranked ids, the first 16 survivors (-1 padded); log_dist [cells, 16] float64 = the first 16 ranked distances.                                      */
#define NERFTEX_ERR_EXHAUSTED 3
#define NERFTEX_SYNTH_CUT 0
#define NERFTEX_SYNTH_BLEND 1
#define NERFTEX_SYNTH_LOG_STRIDE 36
#define NERFTEX_SYNTH_CANVAS 0
#define NERFTEX_SYNTH_CANVAS_ID 1
#define NERFTEX_SYNTH_ID_MAP 2
#define NERFTEX_SYNTH_LOG_IDS 3
#define NERFTEX_SYNTH_LOG_DIST 4
#define NERFTEX_SYNTH_TBN_IDS 5
#define NERFTEX_SYNTH_TBN 6
#define NERFTEX_SYNTH_TOTAL_ID 7
typedef struct nerftex_synth nerftex_synth;
typedef struct nerftex_synth_desc {
    const float* patches;         /* device [P, S, S, C] fp32: features, then phi_embed, then local_tbn                    */
    const float* sample_tbn;      /* device [P, 9]                                                                         */
    const float* picked_vertices; /* device [P, 3]                                                                         */
    uint32_t P, S, C, match_dim;
    uint32_t patch_size, overlap_size;
    uint32_t output_h, output_w;  /* the requested output; the canvas is the next size that holds whole cells              */
    uint32_t mirror_hor, mirror_vert;
    uint32_t attenuation;         /* 3: strict_match, 1: not                                                               */
    uint32_t max_patch_res;       /* 32 in the reference                                                                   */
    uint32_t mode, quilt;         /* NERFTEX_SYNTH_CUT, 0                                                                  */
    double close_threshold;       /* 0.2 in the reference                                                                  */
    double patch_length;          /* S * grid_gap                                                                          */
} nerftex_synth_desc;
typedef struct nerftex_synth_view {
    const float* canvas;          /* [side, side, C]                                                                       */
    const int32_t* canvas_id;     /* [side, side]                                                                          */
    const int32_t* id_map;        /* [cells_per_side^2]                                                                    */
    const int32_t* log_ids;       /* [cells, NERFTEX_SYNTH_LOG_STRIDE]                                                     */
    const double* log_dist;       /* [cells, 16]                                                                           */
    const int32_t* sample_tbn_ids; /* [side, side]                                                                         */
    const float* sample_tbn;      /* [n_total, 9]                                                                          */
    const int32_t* total_id;      /* [n_total]                                                                             */
    uint32_t side, cells_per_side, examples, channels, block, strip_floats, slices, n_total;
} nerftex_synth_view;
int nerftex_synth_create(const nerftex_synth_desc* desc, nerftex_synth** out);
int nerftex_synth_resolve(nerftex_synth* synth, uint32_t first_patch, const double* draws, const int32_t* forced, uint32_t cell_begin, uint32_t cell_end,
                          void* stream);
int nerftex_synth_finish(nerftex_synth* synth, void* stream);
int nerftex_synth_result(const nerftex_synth* synth, nerftex_synth_view* out);
int nerftex_synth_read(const nerftex_synth* synth, uint32_t what, void* dst, size_t bytes, void* stream);
int nerftex_synth_destroy(nerftex_synth* synth);

#ifdef __cplusplus
}
#endif
#endif /* NERFTEX_HIP_H */
