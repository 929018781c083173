/*
 * rvdd.h -- C ABI of librvdd_hip.so, the MI355X (gfx950) runtime for the
 * recurrent video denoise+demosaic inference path of centreborelli/RVDD-release.
 *
 * The reference has no FFI on this path: the path sits behind two string-keyed
 * Python plugin registries (models/__init__.py:25-45 `--model recurrent`,
 * networks/__init__.py:121-176 `--netDenoiser ...`).  This header is what a
 * binding for that plugin surface binds (the ctypes stub is in INTEGRATION.md
 * and rvdd-release_amd/runtime.py).  Conventions mirror the reference's only
 * real FFI, library.CPPbridge (library.py:143-175): plain pointers and sizes,
 * caller-allocated buffers, no exceptions across the boundary.
 *
 *  - every function returns 0 on success or a negative rvdd_status;
 *    rvdd_last_error() gives the message (per handle; NULL -> last create error);
 *  - all tensor pointers are DEVICE pointers to dense fp32 tensors in the
 *    reference's own layout (NCHW), owned by the caller (e.g. obtained from
 *    torch.Tensor.data_ptr() on PyTorch-ROCm).  The one exception: `frames`
 *    of rvdd_ingest_raw / rvdd_video_push, DEVICE pointers to sensor frames
 *    of 16-bit unsigned integers or fp32 in one of the two layouts of
 *    enum rvdd_raw_layout;
 *  - `stream` is a hipStream_t passed as void* (NULL = the default stream);
 *    calls are asynchronous and stream-ordered unless stated otherwise;
 *  - a handle owns its weights, workspace and the recurrent state; one handle
 *    = one device; a handle is not thread-safe, distinct handles are.
 */
#ifndef RVDD_H
#define RVDD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rvdd_handle rvdd_t;

enum rvdd_status {
    RVDD_OK = 0,
    RVDD_ERR_ARG = -1,      /* bad argument / shape */
    RVDD_ERR_STATE = -2,    /* call sequence violated (e.g. step before weights) */
    RVDD_ERR_WEIGHT = -3,   /* unknown / missing / mis-shaped state_dict key */
    RVDD_ERR_HIP = -4,      /* HIP runtime error */
    RVDD_ERR_NOMEM = -5
};

/* Colour-filter layouts of the packed raw frames (util/Hamilton_Adam_demo.py:175-224).  The packing is the same for
 * every pattern: channel k of a [B,4,h,w] frame holds CFA position (k >> 1, k & 1) of each 2x2 cell (pack_in_one,
 * :226-234); the pattern names the colours at the four positions, row by row: GBRG = G B / R G, and so on. */
enum rvdd_bayer {
    RVDD_BAYER_GBRG = 0,    /* the reference model's pattern (models/recurrent_model.py:99); the default */
    RVDD_BAYER_GRBG = 1,
    RVDD_BAYER_RGGB = 2,
    RVDD_BAYER_BGGR = 3
};

/* netDenoiser families (networks/__init__.py:121-176). */
enum rvdd_arch {
    RVDD_ARCH_CONVUNET = 0,       /* convunet-mode=fixedfeatures       networks/unet.py:595-720 */
    RVDD_ARCH_CONVUNET_FEAT = 1,  /* convunet-mode=fixedfeatures+feat  networks/unet.py:725-825 */
    RVDD_ARCH_CONVNEXT = 2,       /* newunet                           networks/new_unet.py:207-362 */
    RVDD_ARCH_CONVNEXT_FEAT = 3   /* newunet-mode=feat                 networks/new_unet.py:365-430 */
};

typedef struct rvdd_cfg {
    int32_t arch;     /* enum rvdd_arch */
    int32_t future;   /* --future_patch_depth: 0 or 1 (options/base_options.py:56) */
    int32_t batch;    /* B sequences advanced in lockstep */
    int32_t height;   /* RGB frame height H (even, >= 16); raw frames are 4 x H/2 x W/2 */
    int32_t width;    /* RGB frame width  W (even, >= 16); H x W x 192 bytes < 2 GiB (11.1 Mpx: 3840 x 2176 fits) */
    int32_t device;   /* HIP device ordinal */
} rvdd_cfg;

/* ---- life cycle ---------------------------------------------------------- */

/* Replaces recurrentModel.__init__ + networks.define_net_arch
 * (models/recurrent_model.py:38-99, networks/__init__.py:121-176). */
int rvdd_create(const rvdd_cfg* cfg, rvdd_t** out);
void rvdd_destroy(rvdd_t* h);
const char* rvdd_last_error(const rvdd_t* h);

/* Replaces BaseModel.load_networks -> net.load_state_dict
 * (models/base_model.py:173-196).  `host` points to HOST fp32 data of one
 * state_dict entry in PyTorch layout (conv weight = OIHW).  Unlike the
 * reference (strict=False) loading is strict: an unknown key fails here, a
 * missing one fails in rvdd_finalize_weights. */
int rvdd_set_weight(rvdd_t* h, const char* key, const float* host, const int64_t* shape, int32_t ndim);
int rvdd_finalize_weights(rvdd_t* h);

/* ---- the recurrent hot path ---------------------------------------------- */

/* FirstOfVideo (validate.py:76-77 -> recurrent_model.py:115,233-245): the next
 * rvdd_step re-initialises lastden from raw_prev and zeroes the features. */
int rvdd_reset(rvdd_t* h);

/* FirstOfVideo per sequence: `mask` (HOST, [cfg.batch] bytes; nonzero = that
 * slot starts a new video) marks slots whose next rvdd_step[_strided]
 * re-initialises lastden from their slice of raw_prev and zeroes their features
 * (and their block-floating-point words); the other slots carry on.  Marks
 * accumulate (OR) until a step that succeeds consumes them; a step that fails
 * leaves them pending.  raw_prev is required on such a step and read only for
 * the marked slots.  A mask of every slot is rvdd_reset (same launches, same
 * bits); an empty mask changes nothing.  Every output of a marked slot is bit
 * for bit what a handle of batch 1 gives for the same video after rvdd_reset,
 * so videos of any length can share a batch.  A mask of some but not all slots
 * needs batch <= 64 (RVDD_ERR_ARG otherwise), and its step runs launch by
 * launch (never replayed from a captured graph). */
int rvdd_reset_slots(rvdd_t* h, const uint8_t* mask);

/* One output frame for each of the B sequences: recurrentModel.set_input +
 * forward, test branch (models/recurrent_model.py:105-135, 161-349):
 * Hamilton-Adams demosaic, flow x2 upsample, bicubic backward warp of the
 * previous output / features / next frame, U-Net forward, state hand-over.
 *   raw_prev, raw_cur, raw_next : [B,4,H/2,W/2] packed raw in the handle's Bayer pattern
 *                                 (rvdd_set_option "bayer_pattern", default GBRG), in [-1,1]
 *                                 (raw_prev is read only on the first step after
 *                                  create/reset, and for the slots rvdd_reset_slots
 *                                  marked; raw_next only when future=1)
 *   flow_prev : [B,2,H/2,W/2] raw-resolution flow cur->prev (x first)
 *   flow_next : [B,2,H/2,W/2] raw-resolution flow cur->next (future=1)
 *   out_rgb   : [B,3,H,W] denoised linear RGB
 */
int rvdd_step(rvdd_t* h, const float* raw_prev, const float* raw_cur, const float* raw_next,
              const float* flow_prev, const float* flow_next, float* out_rgb, void* stream);

/* rvdd_step on channel slices of the reference's own input tensors, without a copy: the model hands the net
 * `n[:, 0:4]`, `n[:, 4:8]`, `n[:, 8:12]` of one [B,(2+f)*4,h,w] tensor and `flow[:, 0]`, `flow[:, 1]` of one
 * [B,1+f,2,h,w] tensor (models/recurrent_model.py:299-324; data/infer4rec_dataset.py:226-230).  Each slice is dense
 * inside a sequence ([4,h,w] / [2,h,w]) and `raw_batch_stride` / `flow_batch_stride` floats apart from one
 * sequence to the next (0 = dense, i.e. 4hw / 2hw as rvdd_step assumes). */
int rvdd_step_strided(rvdd_t* h, const float* raw_prev, const float* raw_cur, const float* raw_next,
                      const float* flow_prev, const float* flow_next, int64_t raw_batch_stride,
                      int64_t flow_batch_stride, float* out_rgb, void* stream);

/* rvdd_step_strided for slots [0, n_live) alone, 1 <= n_live <= cfg.batch: the
 * tensors hold n_live sequences (out_rgb is [n_live,3,H,W]; the strides mean
 * what they mean for rvdd_step_strided) and every launch of the step -- the
 * first-frame latch, the stages in front of the net, both nets, the
 * --prev_noisy_frame hand-over, the launches of a partial reset -- covers
 * n_live sequences.  Choices that depend on a launch's size (which conv kernel
 * "conv_kernel" 4 picks, the one-kernel pre-stage, the output-channel split,
 * "seq_major") are made for n_live, as a handle of that batch makes them.
 * n_live == cfg.batch is rvdd_step_strided: the same launches, the same bits.
 * Every output frame of a live slot is bit for bit what a handle of batch 1
 * gives for that video (the contract of rvdd_reset_slots, extended).
 *
 * Reset marks (rvdd_reset, rvdd_reset_slots) of the live slots are consumed;
 * a mark of a slot >= n_live stays pending.
 *
 * UNDEFINED SLOTS.  A step of n_live < cfg.batch leaves the recurrent state
 * of slots >= n_live undefined: the block-floating-point words rotate through
 * their sets with every step of the handle, so a sequence that sat a step out
 * cannot carry on.  The handle remembers these slots.  A later step that
 * covers one of them without a pending reset mark for it fails with
 * RVDD_ERR_STATE (the message names the slot) and changes nothing; rvdd_reset,
 * a mark of rvdd_reset_slots, rvdd_set_state (with lastden) or being the
 * destination of rvdd_move_slots makes a slot defined again.  Needs batch <= 64
 * when n_live < cfg.batch.  With option "graphs" on, a step of fewer slots
 * runs launch by launch (never replayed from a captured graph). */
int rvdd_step_live(rvdd_t* h, int32_t n_live, const float* raw_prev, const float* raw_cur, const float* raw_next,
                   const float* flow_prev, const float* flow_next, int64_t raw_batch_stride,
                   int64_t flow_batch_stride, float* out_rgb, void* stream);

/* The whole per-sequence state of slot from[k] replaces that of slot to[k],
 * k < count (`from`, `to`: HOST arrays of slot indices): the previous output,
 * the recurrent features, the sequence's block-floating-point words in every
 * set, and the host-side marks (pending reset, undefined).  Slot from[k] is
 * undefined afterwards (see rvdd_step_live) and carries no reset mark.  One
 * kernel launch for all pairs, ordered in `stream`; 208 bytes per pixel read
 * and written per pair.  The pairs must be disjoint -- no slot twice across
 * `from` and `to` -- and inside 0..cfg.batch-1: RVDD_ERR_ARG otherwise, and
 * nothing is moved.  count == 0 does nothing.  Needs batch <= 64.  Together
 * with rvdd_step_live this keeps the live sequences of a pack of videos in
 * the first slots once no video is left to refill a finished one. */
int rvdd_move_slots(rvdd_t* h, const int32_t* from, const int32_t* to, int32_t count, void* stream);

/* Recurrent state in the reference's layout, for get_current_features /
 * set_rec_features parity (networks/unet.py:814-818) and for tests.
 *   lastden  [B,3,H,W]; lastfeat [B,48,H,W] (NULL to skip either). */
int rvdd_get_state(rvdd_t* h, float* lastden, float* lastfeat, void* stream);
int rvdd_set_state(rvdd_t* h, const float* lastden, const float* lastfeat, void* stream);

/* compute_losses, test branch (models/recurrent_model.py:512-525;
 * util/util.py:9-20): out2 (HOST, 2 floats) = { 100*mean|den-gt|,
 * 10*log10(4/mean((den-gt)^2)) } over `count` elements.  Synchronises
 * `stream` (the reference reads the losses back with float(), base_model.py:151). */
int rvdd_psnr_l1(rvdd_t* h, const float* den, const float* gt, int64_t count, float* out2, void* stream);

/* rvdd_psnr_l1 over `n` dense slices of `count` elements each (den / gt
 * [n][count], e.g. one output frame per sequence of a step): out (HOST,
 * [n][2] floats) = { L1*100, PSNR } of each slice, bit for bit what
 * rvdd_psnr_l1 returns for that slice alone.  One batched reduction and one
 * synchronisation of `stream` for all slices; checks a pending asynchronous
 * rvdd_tvl1flow_batch as rvdd_psnr_l1 does.  n = 0 does nothing. */
int rvdd_psnr_l1_batch(rvdd_t* h, const float* den, const float* gt, int32_t n, int64_t count, float* out, void* stream);

/* ---- the same ops one at a time (plugin-level entry points; also test hooks) */

/* netDenoise(x) (networks/unet.py:544-588 / networks/new_unet.py:332-362).
 *   x [B,Cin,H,W] with Cin = 3*(2+future); feat_in/feat_out [B,48,H,W] for the
 *   *_FEAT archs (NULL otherwise); out [B,3,H,W]. */
int rvdd_unet_forward(rvdd_t* h, const float* x, const float* feat_in, float* out, float* feat_out,
                      void* stream);

/* HamiltonAdam('gbrg').forward (util/Hamilton_Adam_demo.py:249-289):
 *   raw [n,4,h,w] -> rgb [n,3,2h,2w].  rvdd_demosaic_ha_bayer with RVDD_BAYER_GBRG. */
int rvdd_demosaic_ha(rvdd_t* h, const float* raw, int32_t n, int32_t hh, int32_t ww, float* rgb,
                     void* stream);

/* HamiltonAdam(pattern).forward (util/Hamilton_Adam_demo.py:175-289) for any of the four patterns (enum
 * rvdd_bayer; any other value is RVDD_ERR_ARG): raw [n,4,h,w] -> rgb [n,3,2h,2w]. */
int rvdd_demosaic_ha_bayer(rvdd_t* h, const float* raw, int32_t n, int32_t hh, int32_t ww, int32_t pattern,
                           float* rgb, void* stream);

/* util.flow_utils.warp(x, flow, "bicubic")[0] (util/flow_utils.py:70-102):
 *   x [n,c,H,W], flow [n,2,H,W] at full resolution -> y [n,c,H,W]. */
int rvdd_warp_bicubic(rvdd_t* h, const float* x, const float* flow, int32_t n, int32_t c, int32_t H,
                      int32_t W, float* y, void* stream);

/* util.flow_utils.upsample_factor_2(t, multiply_by) (util/flow_utils.py:159-174):
 *   t [n,c,hh,ww] -> [n,c,2hh,2ww]. */
int rvdd_upsample_factor_2(rvdd_t* h, const float* t, int32_t n, int32_t c, int32_t hh, int32_t ww,
                           float multiply_by, float* out, void* stream);

/* library.CPPbridge.TVL1_flow -> libBridge `tvl1flow(I0, I1, u, nx, ny)` (libBridge.cpp:44-163): Dual TV-L1
 * optical flow with the reference's hard-wired parameters (3rdparty/tvl1flow/tvl1flow_lib.c:91-278, 343-472).
 *   I0, I1 [ny,nx] gray images; u [2,ny,nx] = x displacement then y displacement (libBridge.cpp:150) such
 *   that I1(x + u) ~ I0(x).  `iterations` (HOST, nullable) receives the total primal-dual iterations run.
 * One cooperative kernel per pyramid scale, all of its blocks resident (csrc/tvl1.hip: since round 4 a block owns a patch of
 * the image and exchanges its perimeter and convergence sum through tagged records that the readers poll -- no grid barrier
 * in the iteration; round 3's barrier kernel is kept, RVDD_TVL1_PATCH=0, and the two are bit-identical, flows and iteration
 * counts).  Synchronous: returns after the flow is complete (the control words are read back to catch an exchange that
 * timed out -- RVDD_ERR_HIP then, never a half-finished flow). */
int rvdd_tvl1flow(rvdd_t* h, const float* I0, const float* I1, float* u, int32_t nx, int32_t ny,
                  int32_t* iterations, void* stream);

/* `n` independent pairs of the same size -- what data/base_dataset.py:134-249 computes one call at a time when it
 * fills the dataset's flow folder.  I0, I1: [n][ny][nx]; u: [n][2][ny][nx]; iterations: HOST [n], nullable.
 * The pairs of a call share launches: the pre-processing and pyramid of all of them, up to eight pairs per scale kernel at
 * the coarse scales, two at 640 x 360 (0.76-0.80 ms per 640 x 360 flow in batches of eight, 1.8-1.9 ms one at a time);
 * every flow is bit-identical to the one rvdd_tvl1flow returns for that pair.  Synchronous. */
int rvdd_tvl1flow_batch(rvdd_t* h, const float* I0, const float* I1, float* u, int32_t n, int32_t nx, int32_t ny,
                        int32_t* iterations, void* stream);

/* ---- raw footage: sensor frames in, denoised frames out --------------------- */

enum rvdd_raw_dtype  { RVDD_RAW_U16 = 0, RVDD_RAW_F32 = 1 };
enum rvdd_raw_layout { RVDD_RAW_MOSAIC = 0,      /* [n,2hh,2ww]: one plane, as a sensor writes it            */
                       RVDD_RAW_PACKED_HWC = 1 };/* [n,hh,ww,4]: the reference dataset's TIFF (iio layout)    */

/* Sensor frames (digital numbers, DN) -> what a frame-step and TV-L1 read, in one kernel:
 *   packed [n,4,hh,ww] = 2 * (dn / (2^bit_depth - 1)) - 1, each operation rounded to f32 on its own and the division
 *          correctly rounded: bit for bit the dataset's transform of library.load_image(path, bit_depth)
 *          (library.py:75-90; data/base_dataset.py define_transforms).  Channel k holds CFA position (k >> 1, k & 1) of each
 *          2x2 cell, packed[k][y][x] = mosaic[2y + (k >> 1)][2x + (k & 1)] -- the packing of enum rvdd_bayer, whatever the
 *          pattern.  No black level is subtracted: the reference leaves it in the data and the checkpoints were trained so.
 *   gray   [n,hh,ww]   = (((c0 + c1) + c2) + c3) * 0.25f of the four DN values of a cell (NOT the normalised ones), an f32
 *          sum in channel order: what library._gray (library.py:118-126, mean over the channels) hands TV-L1.  On
 *          integer-valued frames every summation order gives these bits; on other float frames a reduction that sums in
 *          another order (torch's on the device is free to) may differ in the last bit.
 * Either output may be NULL.  bit_depth 1..16, dtype / layout as the enums: RVDD_ERR_ARG otherwise.  n = 0 does nothing.
 * `frames` 16-byte aligned with ww % 4 == 0 takes the wide form (16-byte accesses, 1 KiB runs per wave). */
int rvdd_ingest_raw(rvdd_t* h, const void* frames, int32_t dtype, int32_t layout, int32_t n, int32_t hh, int32_t ww,
                    int32_t bit_depth, float* packed /* [n,4,hh,ww], nullable */, float* gray /* [n,hh,ww], nullable */,
                    void* stream);

/* The gray plane TV-L1 reads, of an RGB frame's re-mosaic: what rvdd_ingest_raw's `gray` would be for the sensor frame whose
 * demosaic is `rgb`.  For each 2x2 cell (y, x) and CFA position k = 0..3 in the packing of enum rvdd_bayer,
 *   v_k  = rgb[colour of `pattern` at k][2y + (k >> 1)][2x + (k & 1)]     (HamiltonAdam(pattern).remosaick: the inverse of the packing)
 *   dn_k = ((v_k + 1.0f) * 0.5f) * (float)(2^bit_depth - 1)
 *   gray = (((dn_0 + dn_1) + dn_2) + dn_3) * 0.25f
 * every operation rounded to f32 on its own.  The result is in digital numbers, the unit of rvdd_ingest_raw's gray plane: TV-L1
 * normalises a pair with one joint minimum and maximum, so the two images of a pair must share a scale.
 *   rgb [n,3,H,W] in [-1,1] (values outside are not clamped); gray [n,H/2,W/2].
 * pattern 0..3, bit_depth 1..16, H and W even: RVDD_ERR_ARG otherwise (the message names the argument).  n = 0 does nothing.
 * `rgb` and `gray` 16-byte aligned with (W/2) % 4 == 0 takes the wide form (16-byte accesses); same bits either way. */
int rvdd_gray_of_rgb(rvdd_t* h, const float* rgb /* [n,3,H,W] in [-1,1] */, int32_t n, int32_t H, int32_t W,
                     int32_t pattern /* enum rvdd_bayer */, int32_t bit_depth, float* gray /* [n,H/2,W/2] */, void* stream);

enum rvdd_out_layout { RVDD_OUT_RGB_HWC = 0,     /* [n,H,W,3]                                   */
                       RVDD_OUT_MOSAIC = 1,      /* [n,H,W]: one plane, as a sensor writes it    */
                       RVDD_OUT_PACKED_HWC = 2 };/* [n,H/2,W/2,4]: the reference dataset's TIFF  */

/* Denoised frames out, in the containers a raw pipeline reads: the inverse direction of rvdd_ingest_raw.  With
 * top = (float)(2^bit_depth - 1), every operation rounded to f32 on its own,
 *   dn  = ((v + 1.0f) * 0.5f) * top                            (the dn_k of rvdd_gray_of_rgb)
 *   out = dn                                                   RVDD_RAW_F32: neither rounded nor clamped
 *   out = (uint16) min(max(rint(dn), 0), top)                  RVDD_RAW_U16: rint rounds half to even; NaN -> 0, -inf -> 0, +inf -> top
 * of the sample
 *   RVDD_OUT_RGB_HWC     out[i][y][x][c]                      = rgb[i][c][y][x]
 *   RVDD_OUT_PACKED_HWC  out[i][y][x][k]                      = rgb[i][col(k)][2y + (k >> 1)][2x + (k & 1)]
 *   RVDD_OUT_MOSAIC      out[i][2y + (k >> 1)][2x + (k & 1)]  = the same sample
 * where col(k) is the colour `pattern` has at CFA position k (HamiltonAdam(pattern).remosaick, as rvdd_gray_of_rgb).
 * What that gives:
 *   - RGB_HWC, F32, bit_depth 8 is bit for bit util.tensor2im of the frame -- (x.transpose(1,2,0) + 1) / 2.0 * 255.0 in f32 -- the
 *     image validate / denoise write as <frame>_denoised.tif;
 *   - MOSAIC / PACKED_HWC, F32: (((c0 + c1) + c2) + c3) * 0.25f of a cell's four outputs is bit for bit rvdd_gray_of_rgb for the
 *     same pattern and bit_depth;
 *   - the round trip: for uint16 frames with values in 0 .. 2^bit_depth - 1, rvdd_ingest_raw -> rvdd_demosaic_ha_bayer(pattern) ->
 *     rvdd_egress(U16, the same layout, pattern and bit_depth) returns the frames exactly (the demosaic keeps a site's own
 *     sample, and rint(dn_of(packed(dn))) == dn for every dn of every bit_depth: the worst deviation is 9.8e-4 DN, at 16 bits).
 * No black level or white balance is applied: ingest leaves both in the data, and so does this.
 * layout outside 0..2, dtype outside 0..1, bit_depth outside 1..16, H or W < 1, n < 0, NULL rgb / out with n > 0, a launch of
 * more than 2^31 - 1 blocks, and for the two mosaic layouts pattern outside 0..3 or an odd H or W: RVDD_ERR_ARG (the message
 * names the argument) and nothing is launched.  RGB_HWC takes any H, W and ignores pattern.  n = 0 does nothing.
 * Asynchronous and stream-ordered; nothing is read back: after rvdd_video_push, call it on the push's stream.
 * The wide form (every access 16 bytes) needs `rgb` and `out` 16-byte aligned and, for the mosaic layouts, (W/2) % 4 == 0 (a
 * thread owns four cells of a cell row); for RGB_HWC, H * W % 8 == 0 (U16) or H * W % 4 == 0 (F32): a thread owns that many
 * consecutive pixels and stores 3 x 16 bytes.  Every other shape takes the one-cell / one-pixel form; same bits either way. */
int rvdd_egress(rvdd_t* h, const float* rgb /* [n,3,H,W] in [-1,1] */, int32_t n, int32_t H, int32_t W,
                int32_t layout /* enum rvdd_out_layout */, int32_t dtype /* enum rvdd_raw_dtype */,
                int32_t bit_depth, int32_t pattern /* enum rvdd_bayer; ignored for RGB_HWC */,
                void* out, void* stream);

/* Frames of packed 10 / 12 / 14-bit samples, as a sensor or a raw recorder leaves them: a mosaic plane [n,2hh,2ww] whose rows are
 * bit-packed.  Rows are tight and frames are tight -- frame i starts at byte i * 2hh * row_bytes -- and nothing is assumed about
 * alignment; row_bytes may be odd.  With b = bit_depth:
 *   RVDD_BITS_MIPI  MIPI CSI-2 RAW10 / RAW12 / RAW14.  Pixels in groups of G = 4 (b = 10, 14) or 2 (b = 12): G bytes P_k >> (b - 8),
 *                   then G (b - 8) / 8 bytes holding L = sum_k (P_k & (2^(b-8) - 1)) << (k (b - 8)), least significant byte first.
 *                   row_bytes = 2ww b / 8.  2ww must be a multiple of G: ww even for b = 10 and 14.
 *   RVDD_BITS_MSB   TIFF 6.0 with FillOrder 1 / uncompressed DNG.  A row is its samples, b bits each with the most significant bit
 *                   first, as one bit string cut into bytes most significant bit first and zero-padded to a whole byte:
 *                   row_bytes = ceil(2ww b / 8).  Any ww.
 *   e.g. b = 10, pixels 3FF 000 155 2AA: MIPI FF 00 55 AA 93, MSB FF C0 05 56 AA;  b = 12, pixels ABC 123: MIPI AB 12 3C, MSB AB C1 23. */
enum rvdd_bits_order { RVDD_BITS_MIPI = 0, RVDD_BITS_MSB = 1 };

/* rvdd_ingest_raw(RVDD_RAW_U16, RVDD_RAW_MOSAIC, bit_depth) of the frames those bytes hold, in one kernel: `packed` and `gray` are
 * bit for bit what it writes for the unpacked uint16 frames, and no unpacked plane ever exists in memory.  Pad bits (MSB, odd ww)
 * are not read as data, and no byte beyond n * 2hh * row_bytes is read.  Either output may be NULL.
 * order outside 0..1, bit_depth other than 10 / 12 / 14, hh or ww < 1, an odd ww with MIPI at 10 / 14 bits, n < 0, NULL frames with
 * n > 0, a launch of more than 2^31 - 1 blocks: RVDD_ERR_ARG (the message names the argument) and nothing is launched.  n = 0 does
 * nothing.  Asynchronous and stream-ordered; nothing is read back.
 * With ww % 8 == 0, `frames` 4-byte aligned and the outputs 16-byte aligned a thread owns 16 pixels of both sensor rows of a
 * cell row -- 20 / 24 / 28 bytes per row, read as dwords, 16-byte stores; every other case moves single bytes, two cells per
 * thread.  Same bits either way. */
int rvdd_ingest_bits(rvdd_t* h, const uint8_t* frames, int32_t order /* enum rvdd_bits_order */, int32_t n, int32_t hh, int32_t ww,
                     int32_t bit_depth, float* packed /* [n,4,hh,ww], nullable */, float* gray /* [n,hh,ww], nullable */,
                     void* stream);

/* rvdd_egress(RVDD_OUT_MOSAIC, RVDD_RAW_U16, bit_depth, pattern) written as packed bits: the samples are exactly the uint16 values it
 * writes (the same rint and clamp, NaN -> 0, -inf -> 0, +inf -> 2^bit_depth - 1), packed in `order`, pad bits zero.  Every byte of
 * out[0 .. n * H * row_bytes) is written -- row_bytes of W samples, as above -- and nothing outside it.
 * The round trip: for frames with values in 0 .. 2^bit_depth - 1, rvdd_ingest_bits -> rvdd_demosaic_ha_bayer(pattern) ->
 * rvdd_egress_bits(the same order, bit_depth and pattern) returns the input bytes exactly (the uint16 round trip of rvdd_egress;
 * for MSB frames with zero pad bits).
 * order outside 0..1, bit_depth other than 10 / 12 / 14, H or W odd or < 2, W / 2 odd with MIPI at 10 / 14 bits (the message names
 * ww = W / 2), pattern outside 0..3, n < 0, NULL rgb / out with n > 0, a launch of more than 2^31 - 1 blocks: RVDD_ERR_ARG (the message
 * names the argument) and nothing is launched.  n = 0 does nothing.  Asynchronous and stream-ordered; nothing is read back.
 * With W % 16 == 0, `rgb` 16-byte and `out` 4-byte aligned a thread owns 16 pixels of both sensor rows (16-byte loads, dword
 * stores); every other case stores single bytes, two cells per thread.  Same bits either way. */
int rvdd_egress_bits(rvdd_t* h, const float* rgb /* [n,3,H,W] in [-1,1] */, int32_t n, int32_t H, int32_t W,
                     int32_t order /* enum rvdd_bits_order */, int32_t bit_depth, int32_t pattern /* enum rvdd_bayer */,
                     uint8_t* out /* [n,H,row_bytes] */, void* stream);

/* Dynamic defective-pixel correction (DPC) of packed raw frames: hot and stuck samples replaced by the median of their eight
 * same-colour neighbours, on the planes rvdd_ingest_raw / rvdd_ingest_bits write -- packed [n,4,hh,ww] in [-1,1], channel k = CFA
 * position (k >> 1, k & 1).  Inside one channel plane the +-1 neighbours are the same-colour +-2 neighbours of the mosaic, so the
 * rule needs neither the Bayer pattern nor the container.  Every operation is rounded to f32 on its own (no fused multiply-add, no
 * square root): the result is reproducible bit for bit in NumPy f32 (tests/dpc_ref.py).  With top = (float)(2^bit_depth - 1):
 *   dn(v) = ((v + 1) * 0.5) * top                       the dn_k of rvdd_gray_of_rgb
 *   c     = dn(p[k][y][x]); the eight neighbours dn(p[k][y+dy][x+dx]), dy, dx in {-1, 0, 1} not both zero, an index outside the
 *           plane mirrored about the site (-1 -> +1, n -> n - 2: hence hh, ww >= 2)
 *   lo, hi  the smallest and largest neighbour;  m = (s3 + s4) * 0.5, s3 / s4 the 4th / 5th of the eight in ascending order
 *   var   = fmaxf(noise_a * m - noise_b, var_floor)     the noise curve in DN of this bit depth
 *   hot:  k_hot  > 0, d = c - hi > 0 and d * d > (k_hot * k_hot) * var
 *   dead: k_dead > 0, d = lo - c > 0 and d * d > (k_dead * k_dead) * var
 * packed_out: a flagged sample is 2 * (m / top) - 1 (the division correctly rounded: rvdd_ingest_raw's own function), every other
 *   sample a copy of its bits.  A frame in which nothing is flagged is a bit copy.
 * gray [n,hh,ww] (nullable, patched IN PLACE): at a cell in which at least one of the four planes was flagged,
 *   (((d0 + d1) + d2) + d3) * 0.25 with d_k = m_k for a flagged plane (the median in DN, no round trip through the packed value)
 *   and dn(p[k][y][x]) for the others; a cell without a flag is not written.
 * counts (DEVICE uint32 [n,2], nullable): the flags of frame i are ADDED to counts[i][0] (hot) and counts[i][1] (dead).
 * The median of eight tolerates up to three bad neighbours; larger clusters of one colour are out of its reach.  Inputs are assumed
 * finite: with NaN or inf the result is unspecified, but nothing outside the tensors is read or written.
 * RVDD_ERR_ARG (the message names the argument) and nothing launched: NULL cfg; k_hot / k_dead negative or not finite; noise_a /
 * noise_b not finite; var_floor not > 0 (or not finite); bit_depth outside 1..16; hh or ww < 2; n < 0; NULL packed_in / packed_out
 * with n > 0; a launch of more than 2^31 - 1 blocks; packed_out overlapping packed_in.  k_hot = 0 / k_dead = 0 switches that side
 * off.  n = 0 does nothing.  Asynchronous and stream-ordered; nothing is read back.
 * With ww % 4 == 0 and all pointers 16-byte aligned a thread owns four neighbouring cells (16-byte loads and stores); every other
 * case one cell.  Same bits either way. */
typedef struct rvdd_dpc_cfg {
    float k_hot, k_dead;      /* thresholds in standard deviations of the noise curve; 0 = that side off */
    float noise_a, noise_b;   /* var(m) = noise_a * m - noise_b, in DN of the frames' bit depth */
    float var_floor;          /* the least variance assumed, > 0 */
} rvdd_dpc_cfg;
int rvdd_dpc(rvdd_t* h, const float* packed_in /* [n,4,hh,ww] */, float* packed_out /* [n,4,hh,ww] */,
             float* gray /* [n,hh,ww], nullable, patched in place */, int32_t n, int32_t hh, int32_t ww, int32_t bit_depth,
             const rvdd_dpc_cfg* cfg, uint32_t* counts /* DEVICE [n,2], nullable, accumulated */, void* stream);

enum rvdd_push { RVDD_PUSH_NEXT = 0, RVDD_PUSH_FIRST = 1, RVDD_PUSH_IDLE = 2 };

/* The stream: one call hands every batch slot its next sensor frame (`frames`: cfg.batch frames of H/2 x W/2 cells, one
 * per slot, dtype / layout / bit_depth as rvdd_ingest_raw) and enqueues, in stream order, at most one output frame per
 * slot.  Everything between the frames and out_rgb stays on the device; nothing is read back, `stream` is not synchronised.
 *   ctl (HOST [cfg.batch], NULL = all NEXT): FIRST = this frame starts a new video in the slot (its older frames are
 *       forgotten); NEXT = it continues the slot's video; IDLE = the slot gets no frame (its slice of `frames` is not read).
 *       After IDLE a slot goes on with FIRST or IDLE only; NEXT there, or on a slot that never had a FIRST, is
 *       RVDD_ERR_STATE (the message names the slot) and nothing is changed.
 *   valid (HOST [cfg.batch]): 1 for the slots that are READY -- that hold 2 + future frames of their video -- and out_rgb[b]
 *       [cfg.batch,3,H,W] then holds the denoised CENTRE frame: with future = 0 the frame just pushed, with future = 1 the
 *       frame pushed one call earlier.  The outputs of a video of N frames are its frames 1 .. N-1-future, the frames
 *       data/infer4rec_dataset.py yields; option "stream_all_frames" adds frame 0 and, with a future frame, the last frame:
 *       valid[b] is 1 exactly where out_rgb[b] holds an output -- with that option also on a FIRST push (future = 0) and on
 *       an IDLE push (a tail) -- and the frame is the oldest frame of the slot's video not yet output.
 *       out_rgb[b] of a slot without an output is unspecified.
 *   Option "stream_all_frames" (default 0: the paragraph above, the same launches, nothing more allocated).  Let n be the
 *       frames of the slot's video pushed so far, this push included.  A push that carries a frame gives an output iff
 *       n >= 1 + future (not 2 + future), the centre being frame c = n - 1 - future:
 *         c == 0, the HEAD: no previous frame exists, so the step's raw_prev of the slot is frame 0 itself and its flow_prev
 *           all zeros -- by definition: no TV-L1 pair is formed for that direction -- and the step carries the slot's reset
 *           mark.  raw_next / flow_next with a future frame are the ordinary ones (frame 1, TV-L1 of (gray[0], gray[1]); the
 *           noisy pair also under "stream_flow_from_denoised").
 *         c == 1: exactly the first output without the option, its reset mark included: the head's step leaves no trace, and
 *           every output with c >= 1 is bit for bit what the same pushes give with the option off.  Under
 *           "stream_flow_from_denoised" this push keeps the noisy pair: the head's output is not matched against.
 *         c > 1: as without the option.
 *       IDLE on a slot with future = 1 whose previous push carried a frame is the TAIL: it outputs the video's last frame,
 *       c = n - 1 (the slot gets no frame, its slice of `frames` is not read), with raw_next a copy of frame c itself and
 *       flow_next all zeros (no pair); raw_prev / flow_prev are the ordinary ones (under "stream_flow_from_denoised" matched
 *       against the previous output wherever an ordinary push at that position would be).  The recurrence carries on: no
 *       reset mark, except at c == 1 (the video's first regular output) and c == 0 (a one-frame video: head and tail in one
 *       step, previous = next = the frame, both flows zero).  Afterwards the slot is idle as after any IDLE: FIRST or IDLE.
 *       FIRST straight after a video's last frame DROPS that video's tail, as without the option: a caller that wants it
 *       puts one IDLE between two videos of a slot.  With future = 0 there is no tail and IDLE is what it always is.  With
 *       "stream_reset_each" every output carries the reset mark, head and tail included; with "no_warp" no flow exists and
 *       head and tail are just the substituted frames.  A video whose FIRST was pushed with the option off has no head.
 *       The substituted frames are copied inside the slot's ring (one small launch per push that has a FIRST or a tail); a
 *       push whose outputs have no TV-L1 pair at all runs no TV-L1, its step reads a zeroed flow tensor.
 * The handle keeps the last 2 + future ingested frames of every slot (packed and gray) on the device: allocated by the
 * first push, freed with the handle (20 (2 + future) + 24 (1 + future) bytes per raw cell and slot with the flow batch's
 * buffers; 4 more with option "stream_flow_from_denoised", 16 more with rvdd_set_dpc, 3072 bytes per slot with rvdd_set_resid and 10 hh + 24 bytes per slot with rvdd_set_rows, each allocated by the
 * first push that has it on).  For the ready slots a push is exactly the existing path: rvdd_tvl1flow_batch(I0 = gray[centre],
 * I1 = gray[previous]) and, with a future frame, (gray[centre], gray[next]) for all of them in ONE batch call in the form of
 * option "tvl1_async" 1 (whatever the option says), then one rvdd_step_strided on the kept packed frames and those flows.  A
 * slot's first ready push carries its reset mark (rvdd_reset_slots; raw_prev = its oldest frame), so every output is bit for
 * bit what a handle of batch 1 gives for that video.  With option "no_warp" no flow is computed; "warp_raw",
 * "prev_noisy_frame", "bayer_pattern" and the kernel-selection options act inside the step, unchanged.
 * The step has no per-slot skip: slots that are idle or not ready step too, on the finite frames their ring holds and a zero
 * flow (no TV-L1 pair), and their state is re-initialised by the reset mark of their first ready push.  The cost is 1 + future
 * discarded slot-steps per video that starts while others run.  If no slot is ready the push only ingests.
 * Limits, reported as RVDD_ERR_ARG by the first push: cfg.batch <= 64 (the partial marks of rvdd_reset_slots); without
 * "no_warp", frames of at least 16 x 16 cells that rvdd_tvl1flow_batch accepts.
 * A TV-L1 exchange that gave up leaves the batch's control word set, as option "tvl1_async" describes: a streaming loop of
 * pushes never reads it.  It is read -- and reported as RVDD_ERR_HIP -- by rvdd_psnr_l1[_batch], by a TV-L1 call that returns
 * iteration counts, and by rvdd_set_option(h, "tvl1_async", 0), which synchronises the device: call one of them wherever the
 * loop synchronises anyway (python -m rvdd_release_amd.denoise does at the end of every video).
 * rvdd_reset / rvdd_reset_slots / rvdd_step* keep working on such a handle exactly as before: they do not touch the kept
 * frames (and the kept frames do not know of them: a stream goes on from the recurrent state such calls leave). */
int rvdd_video_push(rvdd_t* h, const void* frames /* [B, one frame each] */, int32_t dtype, int32_t layout,
                    int32_t bit_depth, const uint8_t* ctl /* HOST [B], NULL = all NEXT */,
                    float* out_rgb /* [B,3,H,W] */, uint8_t* valid /* HOST [B] */, void* stream);

/* Defective-pixel correction inside rvdd_video_push: cfg = the parameters of rvdd_dpc (checked as there: RVDD_ERR_ARG, the message
 * names the field, and nothing changes), NULL = off, the default.  Its own call and not an rvdd_set_option name because its
 * parameters are floats.  Per handle; acts on rvdd_video_push only; synchronises the device, as rvdd_set_option does.
 * With the stage on a push ingests the packed planes of the slots that get a frame into a scratch tensor [cfg.batch,4,hh,ww]
 * (allocated by the first push that has the stage on: 16 bytes per raw cell and slot, freed with the handle) and their gray planes
 * straight into the ring, then runs rvdd_dpc's kernel from the scratch tensor into the ring's packed frames, patching the ring's
 * gray planes, with the push's bit_depth -- one launch per run of slots that got a frame, as the ingest.  Everything downstream
 * reads the ring as before, so the corrected frames are what TV-L1 matches, what the step denoises and what option
 * "stream_all_frames" copies for a head or a tail (copies of corrected frames: not counted again), under every
 * "stream_container".  With the stage off a push makes exactly the launches it made before and allocates nothing more; a frame in
 * which nothing is flagged leaves the ring bit for bit what a push without the stage leaves. */
int rvdd_set_dpc(rvdd_t* h, const rvdd_dpc_cfg* cfg /* NULL = off, the default */);

/* The samples the stage corrected, per batch slot, since rvdd_set_dpc last switched it ON (off -> on; a call that only changes the
 * parameters keeps the totals): hot_dead[b][0] hot, hot_dead[b][1] dead.  Copies the device's counters to the host on `stream` and
 * synchronises it: call it where the loop synchronises anyway.  All zeros on a handle that never had the stage on. */
int rvdd_dpc_counts(rvdd_t* h, uint64_t* hot_dead /* HOST [cfg.batch,2] */, void* stream /* synchronised */);

/* The static defect map: the sites of persistent defects found once, then those sites and only those corrected.  A real defect sits
 * at the same site in every frame while scene detail moves, so rvdd_dpc's rule is COUNTED per site over frames spread across the
 * footage (rvdd_dpc_detect), the counts are thresholded on the host into a map, and the map is applied by rvdd_dpc_map_apply or as a
 * stage of rvdd_video_push (rvdd_set_dpc_map).  dn(v), top, norm_dn(d) = 2 * (d / top) - 1 and the mirroring of the eight neighbours
 * are rvdd_dpc's; every operation is rounded to f32 on its own, so every integer and every written value is reproducible bit for bit
 * in NumPy (tests/dpc_map_ref.py).
 *
 * rvdd_dpc_detect.  Per sample of packed [n,4,hh,ww]: the eight neighbours of rvdd_dpc in ascending order s0 .. s7,
 * m = (s3 + s4) * 0.5, var = fmaxf(noise_a * m - noise_b, var_floor) with the fields of cfg->rule, and with t = cfg->tolerate (0..3):
 *   hot:  k_hot  > 0, d = c - s[7 - t] > 0 and d * d > (k_hot * k_hot) * var
 *   dead: k_dead > 0, d = s[t] - c > 0 and d * d > (k_dead * k_dead) * var
 * t = 0 is exactly rvdd_dpc's decision.  t > 0 also finds the members of clusters with at most t other defects among a site's eight
 * same-colour neighbours (the median bears three).  It is meant for flat or dark calibration footage: on texture t > 0 flags edges
 * and thin lines, where a sample legitimately stands above all but t of its neighbours.
 * hits (DEVICE uint32 [4,hh,ww], the caller zeroes it before the first call): hits[k][y][x] holds the site's hot frames in its low 16
 * bits and its dead frames in its high 16; the n frames of a call are ADDED, each half on its own, saturating at 65535.  One thread
 * owns a site across the n frames and updates its word with a plain load, add and store -- no atomics -- and calls are
 * stream-ordered, so the totals do not depend on how the frames are split over calls.
 * RVDD_ERR_ARG (the message names the argument) and nothing launched: NULL cfg; the fields of cfg->rule as in rvdd_dpc; tolerate
 * outside 0..3; reserved != 0; bit_depth outside 1..16; hh or ww < 2; n < 0; NULL hits; NULL packed with n > 0; a launch of more than
 * 2^31 - 1 blocks.  n = 0 does nothing.  Asynchronous and stream-ordered; nothing is read back.
 * With ww % 4 == 0 and both pointers 16-byte aligned a thread owns four neighbouring sites (16-byte loads and stores); every other
 * case one site.  Same integers either way. */
typedef struct rvdd_dpc_detect_cfg {
    rvdd_dpc_cfg rule;        /* the thresholds and the noise curve, as rvdd_dpc takes them */
    int32_t tolerate;         /* 0..3: other defects among the eight neighbours a site may have and still be found */
    int32_t reserved;         /* 0 */
} rvdd_dpc_detect_cfg;
int rvdd_dpc_detect(rvdd_t* h, const float* packed /* [n,4,hh,ww] */, int32_t n, int32_t hh, int32_t ww, int32_t bit_depth,
                    const rvdd_dpc_detect_cfg* cfg, uint32_t* hits /* DEVICE [4,hh,ww], accumulated; caller zeroes */, void* stream);

/* The map.  cellmask, uint8 [hh,ww]: bit k (0..3) is set where plane k of the cell -- CFA position (k >> 1, k & 1) -- is defective;
 * bits 4..7 must be zero.  (On disk it is a one-sample uint8 image of the mosaic [2hh,2ww], nonzero = defective, whatever the Bayer
 * pattern: python -m rvdd_release_amd.dpc_map writes it.)
 * The correction of a defective sample of plane k at (y, x).  An index that leaves the plane is reflected about its edge (-i -> i,
 * n - 1 + i -> n - 1 - i; for ring 1 that is rvdd_dpc's mirroring), hence hh, ww >= 3.  Ring 1 is the eight neighbours, ring 2 the
 * sixteen sites of the border of the 5 x 5 window, dy outer and dx inner, ascending.  A site is GOOD iff bit k of cellmask at its
 * reflected index is clear.  Of the first ring that has a good site, with q good values in DN in ascending order s0 .. s(q-1):
 *   rep = (s[(q - 1) / 2] + s[q / 2]) * 0.5, and the sample becomes norm_dn(rep).
 * If neither ring has a good site the sample is UNFIXABLE: it keeps its bits.
 * gray (nullable), at every cell of the map: (((d0 + d1) + d2) + d3) * 0.25 with d_k = rep for a corrected plane and dn(p[k][y][x])
 * for every other one (rvdd_dpc's convention); cells outside the map are not written.
 *
 * rvdd_dpc_map_stats: out3 = {defective samples, defective cells, unfixable samples} of a map, by the rule above, on the host -- it
 * needs neither a handle nor a device (the error string is rvdd_last_error(NULL)'s).  RVDD_ERR_ARG: NULL cellmask / out3, hh or
 * ww < 3, a bit above bit 3. */
int rvdd_dpc_map_stats(const uint8_t* cellmask /* HOST [hh,ww] */, int32_t hh, int32_t ww,
                       int64_t* out3 /* samples, cells, unfixable samples */);

/* The handle's map: uploads the mask and the ascending list of its defective cells (device memory owned by the handle: hh * ww bytes
 * and 4 bytes per defective cell, freed by the next call and with the handle).  NULL = off, the default.  An empty map is valid.
 * Synchronises the device, as rvdd_set_dpc does.  RVDD_ERR_ARG and the map stays what it was: hh or ww < 3, hh * ww >= 2^31, a bit
 * above bit 3.
 * As a stage of rvdd_video_push: with a map set, the frames of every run of slots that got a frame are corrected in place right
 * behind their ingest -- without rvdd_set_dpc in the ring, with rvdd_set_dpc in its scratch tensor (the gray planes in the ring)
 * BEFORE rvdd_dpc's kernel, so that the dynamic rule sees cleaned neighbours; rvdd_set_match's map comes after both.  Every output
 * is bit for bit rvdd_ingest_raw -> rvdd_dpc_map_apply -> (rvdd_dpc) -> flows -> rvdd_step on a handle of batch 1, under every
 * "stream_container" and under "stream_all_frames" (copies of corrected frames).  A push of another frame size than the map's is
 * RVDD_ERR_ARG.  With the map off -- or empty -- a push makes exactly the launches it made before, and nothing more is allocated. */
int rvdd_set_dpc_map(rvdd_t* h, const uint8_t* cellmask /* HOST [hh,ww]; NULL = off, the default */, int32_t hh, int32_t ww);

/* The handle's map applied to packed frames IN PLACE (and to their gray planes, nullable).  Only good sites are read and only
 * defective ones written, so there is no scratch tensor and no race, and applying the map twice gives the bits of applying it
 * once.  One thread per (frame, defective cell), the only owner of the cell's four planes and its gray value: the cost follows the
 * number of defects, not the frame size.  An empty map, or n = 0, launches nothing.
 * RVDD_ERR_ARG (the message names the argument), nothing launched: bit_depth outside 1..16, hh or ww < 3, n < 0, NULL packed with
 * n > 0, a launch of more than 2^31 - 1 blocks.  RVDD_ERR_STATE: no map set, or a map of another hh x ww.  Asynchronous and
 * stream-ordered; nothing is read back. */
int rvdd_dpc_map_apply(rvdd_t* h, float* packed /* [n,4,hh,ww], IN PLACE */, float* gray /* [n,hh,ww], nullable, in place */,
                       int32_t n, int32_t hh, int32_t ww, int32_t bit_depth, void* stream);

/* The sensor's noise curve var(m) = a * m - b (what rvdd_dpc_cfg's noise_a / noise_b ask for) estimated from the footage itself:
 * rvdd_noise_hist gathers block statistics of packed frames into a histogram on the device, rvdd_noise_fit fits the curve to a host
 * copy of it.  The rule, on packed [n,4,hh,ww] in [-1,1] as rvdd_ingest_raw / rvdd_ingest_bits / rvdd_dpc write it, with
 * top = (float)(2^bit_depth - 1) and dn(v) = ((v + 1) * 0.5) * top as in rvdd_dpc, every operation rounded to f32 on its own (no fused
 * multiply-add), so that every integer below is reproducible in NumPy (tests/noise_ref.py):
 *   blocks  each channel plane is cut into 8 x 8 blocks anchored at (0, 0): hh / 8 x ww / 8 whole blocks; rows and columns beyond
 *           the last whole block are ignored; hh < 8 or ww < 8 gives zero blocks, which is valid.
 *   per block, x[r][c] = dn(sample):
 *     rs_r = ((((((x[r][0] + x[r][1]) + x[r][2]) + ...) + x[r][7]);  s = ((rs_0 + rs_1) + ...) + rs_7;  m = s * (1/64)
 *     d    = x[r][c] - (x[r][c-1] + x[r][c+1]) * 0.5 for c = 1..6: a horizontal second difference, which cancels linear ramps and
 *            has variance 1.5 sigma^2;  rq_r = the sum of d * d over c = 1..6 in that order, from 0;  q = ((rq_0 + rq_1) + ...) + rq_7
 *     v    = q * (float)(1.0 / 72.0)                          the block's variance estimate
 *   a block is CLIPPED if any of its 64 samples is <= 0 or >= top in DN, DEGENERATE if it is not clipped and v == 0; neither enters
 *   the histogram.  Every other block adds one to hist[i][j] and (int64)rint(m * 16) to msum[i]:
 *     i = (int)(m * (64 / 2^bit_depth))                       the mean bin, 0..63 (the scale is a power of two)
 *     j = clamp((bits(v) >> 19) - ((127 - 6) << 4), 0, 511)   the exponent and the top four mantissa bits of v: 16 sub-bins per
 *                                                             octave from 2^-6 to 2^26, integer work only
 *   counters = { blocks seen, clipped, degenerate, 0 }.
 * Every add is an integer atomic, so the totals do not depend on the order of arrival: two runs give the same bits, and a batch in
 * one call gives what its halves give in two.  Inputs are assumed finite: which counts a block with a NaN or an inf adds to is
 * unspecified, but both keys are clamped, and nothing outside the tensors is read or written whatever the input. */
typedef struct rvdd_noise_acc {
    uint32_t hist[64][512];   /* [mean bin][variance sub-bin] */
    uint64_t msum[64];        /* sum of (int64)rint(m * 16) over the blocks of the mean bin */
    uint64_t counters[4];     /* blocks seen, clipped, degenerate, reserved (0) */
} rvdd_noise_acc;

/* Adds the blocks of `packed` to *acc (DEVICE, 131616 bytes, 8-byte aligned; the caller zeroes it once and may accumulate any
 * number of calls, frame sizes and videos of one bit depth into it).  One kernel, a lane per block; equal keys are combined in a
 * table in the workgroup's LDS, so that a flat scene, whose blocks all share a handful of keys, issues one atomic per distinct key
 * and workgroup.  With ww % 4 == 0 and `packed` 16-byte aligned a row of a block is two 16-byte loads, single floats otherwise:
 * same integers either way.
 * RVDD_ERR_ARG (the message names the argument) and nothing launched: NULL acc, or one not 8-byte aligned; bit_depth outside 1..16; n, hh or ww < 0; NULL packed
 * with n > 0 and at least one block; a launch of more than 2^31 - 1 workgroups.  n = 0 or zero blocks does nothing.  Asynchronous
 * and stream-ordered; nothing is read back. */
int rvdd_noise_hist(rvdd_t* h, const float* packed /* [n,4,hh,ww] */, int32_t n, int32_t hh, int32_t ww, int32_t bit_depth,
                    rvdd_noise_acc* acc /* DEVICE, accumulated; caller zeroes */, void* stream);

/* The fit, in f64 on the host; needs neither a device nor a handle (errors go where rvdd_create's go: rvdd_last_error(NULL)).
 *   usable bins: the mean bins i with count_i = sum_j hist[i][j] >= 16;  m_i = msum[i] / 16 / count_i
 *   v_i = the lower quartile of row i of the histogram / C_Q: the first sub-bin j at which the cumulative count reaches
 *         0.25 * count_i, interpolated linearly inside it between its edges -- the edge of sub-bin j is the f32 whose bits are
 *         (j + ((127 - 6) << 4)) << 19 -- and divided by C_Q = 0.8051, the lower quartile of the rule's v on unit white Gaussian samples
 *         (tools/noise_cq.py).  The lower quartile and not the mean or the median because texture only ever raises v: with a third
 *         of the blocks textured the predicted sigma comes out a few per cent high, about half of what the median gives; an
 *         over-estimate is the safe side for rvdd_dpc.
 *   a, b: weighted least squares of v = a * m - b over the usable bins with weights count_i / v_i^2
 *   rms = sqrt(sum_i count_i ((v_i - (a m_i - b)) / v_i)^2 / sum_i count_i)
 * RVDD_ERR_ARG: NULL acc_host / out, bit_depth outside 1..16.  RVDD_ERR_STATE, *out untouched, when fewer than 4 bins are usable or
 * their means span less than 2^bit_depth / 16: the message says which (the footage has too little tonal range, or too few frames).
 * The estimate assumes one camera setting -- one gain, one curve -- for everything accumulated. */
typedef struct rvdd_noise_curve {
    double a, b;              /* var(m) = a * m - b in DN of bit_depth */
    double m_min, m_max;      /* the smallest and largest bin mean used, DN */
    double rms;               /* weighted RMS of the relative residuals */
    uint64_t blocks;          /* blocks in the usable bins */
    int32_t bins;             /* usable bins */
    int32_t reserved;         /* 0 */
} rvdd_noise_curve;
int rvdd_noise_fit(const rvdd_noise_acc* acc_host /* HOST copy */, int32_t bit_depth, rvdd_noise_curve* out);

/* ---- scene cuts: one small integer signature per frame ------------------------ */

/* Where one shot ends and the next begins, so that a reel can be streamed shot by shot (RVDD_PUSH_FIRST at every cut) and the recurrence
 * never aligns two unrelated images: rvdd_frame_sigs measures every frame on the device, rvdd_cut_score compares two measurements on the
 * host.  The rule, on gray [n,hh,ww] -- the plane rvdd_ingest_raw / rvdd_ingest_bits write: f32, in DN of bit_depth -- with
 * top = (float)(2^bit_depth - 1), every operation rounded to f32 on its own (no fused multiply-add), so that every integer below is
 * reproducible in NumPy (tests/cuts_ref.py).  Per cell g = gray[i][y][x]:
 *   c  = fminf(fmaxf(g, 0), top)
 *   q  = (uint32) rintf(c * 4.0f)                    0 .. 4 * top, exact: gray is a mean of four DN; ties round to even
 *   j  = min((int)(c * (64 / 2^bit_depth)), 63)      the level bin (the scale is a power of two, as rvdd_noise_hist's mean bin)
 *   by = (16 * y) / hh,  bx = (16 * x) / ww          integer division (in 64 bits): 16 bands of rows x 16 columns; hh, ww >= 16, so
 *                                                    that every band and every column holds at least one cell
 *   hist[by][j] += 1;   sum[by][bx] += q
 * Integer sums only, so the result does not depend on the order of summation: two runs give the same bits, and a batch gives what
 * its frames give one at a time.  With NaN or inf in the input the counts are unspecified (as it happens fmaxf / fminf put NaN at 0
 * and inf at an end of the range), but nothing outside the tensors is read or written. */
typedef struct rvdd_frame_sig {   /* 6144 bytes */
    uint32_t hist[16][64];        /* [band][level bin]: cells */
    uint64_t sum[16][16];         /* [band][column]: sum of q */
} rvdd_frame_sig;

/* sig[i] = the signature of gray[i], every word of it OVERWRITTEN (the caller need not clear anything; nothing beyond sig[n - 1] is
 * touched).  One kernel, one workgroup per (frame, band): every word of the struct has exactly one owner, which reads its band's rows
 * -- a contiguous run of the plane --, counts in its LDS and writes its 64 + 16 words with plain stores.  No global atomics.  With
 * ww % 4 == 0 and `gray` 16-byte aligned the rows are read with 16-byte loads, single floats otherwise: same integers either way.
 * RVDD_ERR_ARG (the message names the argument) and nothing launched: bit_depth outside 1..16; hh or ww < 16; n < 0; NULL gray or
 * sig with n > 0; sig not 8-byte aligned; a launch of more than 2^31 - 1 blocks (16 n).  n = 0 does nothing.  Asynchronous and
 * stream-ordered; nothing is read back. */
int rvdd_frame_sigs(rvdd_t* h, const float* gray /* [n,hh,ww] */, int32_t n, int32_t hh, int32_t ww, int32_t bit_depth,
                    rvdd_frame_sig* sig /* DEVICE [n], 8-byte aligned, OVERWRITTEN */, void* stream);

/* How far two frames of hh x ww cells lie apart, from HOST copies of their signatures; f64 on the host, needs neither a device nor a
 * handle (errors go where rvdd_noise_fit's go: rvdd_last_error(NULL)).  With H_a[j] = sum over the bands of a.hist[band][j] and
 * N = hh * ww:
 *   out2[0] = d_hist = sum_j |H_a[j] - H_b[j]| / (2 N)                                        in [0,1]: how much of the level histogram moved
 *   out2[1] = d_grid = sum_blocks |a.sum - b.sum| / max(1, sum_blocks max(a.sum, b.sum))      in [0,1]: how much of the 16 x 16 layout moved
 * Numerators and denominators are integer sums, converted to f64 once each: the same formulas on Python integers give the same bits.
 * RVDD_ERR_ARG and *out2 untouched: NULL a / b / out2; hh or ww < 16; sum_j H[j] != N for either signature (the message says which:
 * signatures of another frame size).
 * A caller declares a cut where d_hist or d_grid exceeds a threshold (python -m rvdd_release_amd.cuts: 0.10 and 0.12; DESIGN.md 4.17
 * says what those rest on, and that none of it is measured on real footage). */
int rvdd_cut_score(const rvdd_frame_sig* a /* HOST */, const rvdd_frame_sig* b /* HOST */, int32_t hh, int32_t ww,
                   double* out2 /* HOST { d_hist, d_grid } */);

/* ---- footage matched to the checkpoint's noise curve ------------------------- */

/* The checkpoints were trained on two noise curves of one synthetic camera (in 12-bit DN: ISO 3200 var = 8.0034 m - 2043.51144, ISO
 * 12800 var = 28.3015 m - 6307.62081).  An affine curve maps onto any other affine curve by an affine map of the samples: with
 * x' = s x + t the variance of x' is s^2 (a x - b) = (s a) x' - (s a t + s^2 b), so s = a_ref / a and t = (b_ref - s^2 b) / a_ref give
 * exactly the curve (a_ref, b_ref), and the black level comes along, since b is about a * black.  On samples in [-1,1], where
 * x = ((v + 1) / 2) * 4095 in 12-bit DN whatever the bit depth, that map is
 *   v' = scale * v + offset,   scale = s,   offset = s - 1 + 2 t / 4095.
 * Pointwise, no weights; the network sees footage with the statistics it was trained on, its output is mapped back.
 * Footage NOISIER than the checkpoint's curve (s < 1) is compressed into the trained range: the case the map is for.  Footage CLEANER than
 * the curve (s > 1) is stretched by s beyond the trained range and can lose quality (DESIGN.md 4.16 has the measured table). */
typedef struct rvdd_match_cfg {
    float scale, offset;      /* v' = scale * v + offset on samples in [-1,1]; scale finite and > 0, offset finite */
} rvdd_match_cfg;

/* The coefficients, in f64 on the host; needs neither a device nor a handle (errors go where rvdd_noise_fit's go:
 * rvdd_last_error(NULL)).  a, b: the footage's curve in DN of bit_depth, what rvdd_noise_fit returns; a_ref, b_ref: the checkpoint's
 * curve in 12-bit DN.  Each operation as written, in this order:
 *   k = 4095 / (2^bit_depth - 1);  a12 = k * a;  b12 = (k * k) * b;  s = a_ref / a12;  t = (b_ref - (s * s) * b12) / a_ref
 *   out->scale = (float)s;  out->offset = (float)((s - 1) + (2 * t) / 4095)
 * s_t (nullable): { s, t } with t in 12-bit DN.  A reference curve matched onto itself at 12 bits gives scale = 1, offset = 0 exactly.
 * RVDD_ERR_ARG and *out untouched: NULL out; a or a_ref not finite or not > 0; b or b_ref not finite; bit_depth outside 1..16;
 * coefficients that are not finite (or a scale that is not > 0) once rounded to f32. */
int rvdd_match_coeffs(double a, double b, int32_t bit_depth, double a_ref, double b_ref, rvdd_match_cfg* out,
                      double* s_t /* HOST [2], nullable */);

/* The map on packed frames [n,4,hh,ww] (as rvdd_ingest_raw / rvdd_ingest_bits / rvdd_dpc write them): out = (scale * v) + offset,
 * two f32 operations each rounded on its own (no fused multiply-add), reproducible bit for bit in NumPy f32 (tests/match_ref.py).
 * packed_out == packed_in (in place) is allowed; any other overlap is RVDD_ERR_ARG.  Gray planes are not this call's business: TV-L1
 * keeps matching the sensor's own planes.
 * With both pointers 16-byte aligned and the element count a multiple of 4 a thread owns four samples (16-byte loads and stores),
 * every other case one sample.  Same bits either way.
 * RVDD_ERR_ARG (the message names the argument) and nothing launched: NULL cfg; scale not finite or not > 0; offset not finite;
 * n < 0; hh or ww < 1; NULL packed_in / packed_out with n > 0; a launch of more than 2^31 - 1 blocks; a partial overlap.  n = 0 does
 * nothing.  Asynchronous and stream-ordered; nothing is read back. */
int rvdd_match_raw(rvdd_t* h, const float* packed_in /* [n,4,hh,ww] */, float* packed_out /* [n,4,hh,ww], may be packed_in */,
                   int32_t n, int32_t hh, int32_t ww, const rvdd_match_cfg* cfg, void* stream);

/* The way back on network outputs [n,3,H,W]: out = (v - offset) * r with r = (float)(1.0 / (double)scale) formed once on the host;
 * the difference and the product each rounded to f32 on their own.  In place, forms, errors (H or W < 1) and semantics as
 * rvdd_match_raw.  A sample of an integer DN of up to 16 bits that goes through rvdd_match_raw and back lands within a small
 * fraction of a DN of itself, so rvdd_egress's rounding returns the DN (tests/test_match_host.py walks every DN). */
int rvdd_unmatch_rgb(rvdd_t* h, const float* rgb_in /* [n,3,H,W] */, float* rgb_out /* [n,3,H,W], may be rgb_in */, int32_t n,
                     int32_t H, int32_t W, const rvdd_match_cfg* cfg, void* stream);

/* The map as a stage of rvdd_video_push: cfg = the coefficients (checked as rvdd_match_raw checks them: RVDD_ERR_ARG, the message
 * names the field, and nothing changes), NULL = off, the default.  Its own call like rvdd_set_dpc, because its parameters are floats.
 * Per handle; acts on rvdd_video_push only; synchronises the device.  With the stage on a push
 *   - maps the ring's packed frames of the slots that got a frame, in place, after the ingest and after rvdd_set_dpc's correction (which
 *     keeps working in the sensor's domain with the sensor's curve): one launch per run of slots, as the ingest.  The gray planes stay
 *     the sensor's, so TV-L1 matches what it matches without the stage.  The copies option "stream_all_frames" makes for a head or a
 *     tail are copies of mapped frames and are not mapped again;
 *   - maps out_rgb back in place after the step, all cfg.batch slots in one launch, BEFORE option "stream_flow_from_denoised" takes its
 *     gray plane from it: that plane is in the sensor's domain like the ring's gray planes it is paired with.
 * The recurrent state stays in the mapped domain: it is the network's own.  out_rgb is in the sensor's domain, so rvdd_egress and
 * everything behind it need nothing new.  Every output is bit for bit rvdd_ingest_raw -> rvdd_match_raw -> the flows of the un-mapped
 * gray planes -> rvdd_step -> rvdd_unmatch_rgb on a handle of batch 1.  The stage allocates nothing; with it off a push makes exactly the
 * launches it made before.  Switch it between videos: frames mapped with other coefficients stay in the ring as they are. */
int rvdd_set_match(rvdd_t* h, const rvdd_match_cfg* cfg /* NULL = off, the default */);

/* ---- denoised footage checked without ground truth: residual statistics -------- */

/* If the output is the clean frame, then noisy - remosaic(denoised) is the noise: its variance at level m is a * m - b, its mean is
 * zero, and neighbouring samples of one colour plane are uncorrelated.  Variance below the curve means noise left in the output (or a
 * curve that was over-estimated); variance above it together with a positive neighbour correlation means scene detail removed; a
 * mean away from zero means a level shift.  rvdd_resid_stats reduces a frame pair to 3072 bytes of integers on the device,
 * rvdd_resid_fit judges a host copy of them against a curve.
 * What the numbers can and cannot tell (DESIGN.md 4.19 has the measured table, synthetic sequences with ground truth, three seeds): the
 * output is never the clean frame, so the matched baseline is not ratio 1 and not one number -- 1.80-1.82 with rho 0.26-0.36 for the ISO 3200
 * checkpoint, 1.17-1.20 with rho 0.09-0.12 for the ISO 12800 one -- and a report is read against the matched run of the same family.
 * Against that, ratio separates the wrong family, a match curve off by a factor 2 either way and footage of half or double the gain;
 * it does not rank quality, it barely moves (1.23 against 1.17-1.20) for the one case that loses 7.7 dB, and a black level off by 16 DN
 * shows as a lower ratio_lo, not in bias, because the network follows the level.  Nothing is measured on real footage.
 * The rule, on packed [n,4,hh,ww] (the noisy frames as rvdd_ingest_raw / rvdd_dpc / rvdd_match_raw leave them) and rgb [n,3,2hh,2ww]
 * (the outputs for them), with top = (float)(2^bit_depth - 1), dn(v) = ((v + 1) * 0.5) * top and S = 2^(15 - bit_depth) (1/8 DN at 12
 * bits), every operation rounded to f32 on its own (no fused multiply-add) and every sum an integer, so that every word below is
 * reproducible bit for bit in NumPy (tests/resid_ref.py).  Per plane k = 0..3 and cell (y, x):
 *   c  = dn(packed[k][y][x])
 *   d  = dn(rgb[col(k)][2y + (k >> 1)][2x + (k & 1)])      col(k): the colour of `pattern` at CFA position k (rvdd_gray_of_rgb's v_k)
 *   rq = (int)rintf(fminf(fmaxf((c - d) * S, -2^17), 2^17))  the residual in units of 1 / S DN, clamped (ties round to even)
 *   dc = fminf(fmaxf(d, 0), top)
 *   j  = min((int)(dc * (64 / 2^bit_depth)), 63)           the level bin of the DENOISED value (rvdd_frame_sigs' power-of-two scale)
 *   n[j] += 1;  msum[j] += (uint64)rintf(dc * 16);  s1[j] += rq;  s2[j] += rq * rq
 *   and where x < ww - 1:  n11[j] += 1;  s11[j] += rq(x) * rq(x + 1)   the right neighbour of the same plane and row; binned by j of x
 * All sums wrap modulo 2^64.  Real frames stay far below that: rq * rq is below 2^34 at the clamp and below 2^24 for a residual of
 * 500 DN at 12 bits, so one bin holds 2^40 such samples -- thirty thousand frames of 3840 x 2160 sites that all fall into it -- and an
 * accumulator lives for one shot.  With NaN or inf in an input the counts are unspecified (as it happens fmaxf / fminf put NaN at an
 * end of the range), but both j and rq are clamped and nothing outside the tensors is read or written. */
typedef struct rvdd_resid_acc {   /* 3072 bytes */
    uint64_t n[64];               /* samples in level bin j */
    uint64_t msum[64];            /* sum of (uint64)rintf(dc * 16) */
    int64_t  s1[64];              /* sum of rq */
    uint64_t s2[64];              /* sum of rq * rq */
    uint64_t n11[64];             /* pairs (x < ww - 1) */
    int64_t  s11[64];             /* sum of rq(x) * rq(x + 1) */
} rvdd_resid_acc;

/* The sums of frame i are ADDED to acc[i] (DEVICE, n structs, 8-byte aligned; the caller zeroes them once): one accumulator per frame,
 * integer atomics, so a batch gives what its frames give one at a time whatever the order of arrival, and calls accumulate.  One
 * kernel.  With ww % 4 == 0 and `packed` and `rgb` 16-byte aligned a thread owns four neighbouring cells (16-byte loads of the four
 * planes and of the two RGB rows they need), one cell otherwise: same integers either way.  Equal bins are combined inside the wave
 * before LDS is touched, the workgroup's 64 x 6 table is folded into acc[i] with one 64-bit atomic per non-zero word, and a frame is
 * walked by at most 128 workgroups, so that a flat frame -- one bin -- costs what a scene costs.
 * RVDD_ERR_ARG (the message names the argument) and nothing launched: pattern outside 0..3; bit_depth outside 1..16; hh or ww < 1;
 * n < 0; NULL packed / rgb / acc with n > 0; acc not 8-byte aligned; a launch of more than 2^31 - 1 blocks.  n = 0 does nothing.
 * Asynchronous and stream-ordered; nothing is read back. */
int rvdd_resid_stats(rvdd_t* h, const float* packed /* [n,4,hh,ww] */, const float* rgb /* [n,3,2hh,2ww] */, int32_t n, int32_t hh,
                     int32_t ww, int32_t pattern /* enum rvdd_bayer */, int32_t bit_depth,
                     rvdd_resid_acc* acc /* DEVICE [n], 8-byte aligned, accumulated; caller zeroes */, void* stream);

/* The judgement against the curve var(m) = a * m - b (DN of bit_depth), in f64 on the host; needs neither a device nor a handle
 * (errors go where rvdd_noise_fit's go: rvdd_last_error(NULL)).  Each operation as written, sums over the bins in ascending j, so
 * that the same formulas in Python floats give the same numbers (tests/resid_ref.py).  With S = 2^(15 - bit_depth):
 *   usable bins: n[j] >= 1024 and p_j = a * m_j - b > 0, where m_j = msum[j] / 16 / n[j]
 *   per usable bin: u_j = s1[j] / n[j] / S;  var_j = s2[j] / n[j] / (S * S) - u_j * u_j;  ratio_j = var_j / p_j
 *   ratio    = (sum of n[j] * ratio_j) / (sum of n[j]) over the usable bins; `samples` is that sum of n[j], `bins` their number
 *   ratio_lo = the same mean over the darkest third of the usable samples: walking the usable bins upwards with T = samples / 3 and
 *              c = 0, a bin weighs w = min(n[j], T - c) while w > 0, then c += w (the bin that straddles T counts in part);
 *   ratio_hi = the same, walking downwards: the brightest third
 *   bias     = SUM s1 / SUM n / S                        in DN; the SUMs here and in rho are exact integer sums over ALL 64 bins,
 *   rho      = (SUM s11 / SUM n11) / (SUM s2 / SUM n)    each converted to f64 once; 0 where SUM n11 or SUM s2 is 0
 *   a_fit, b_fit: weighted least squares of var_j = a_fit * m_j - b_fit over the usable bins with var_j > 0, weights n[j] / var_j^2,
 *              centred exactly as rvdd_noise_fit's; both 0 where fewer than 2 such bins exist or their m_j do not differ
 * RVDD_ERR_ARG: NULL acc_host / out, bit_depth outside 1..16, a or b not finite.  RVDD_ERR_STATE, *out untouched, when fewer than 4
 * bins are usable (too few frames, or a curve that predicts no noise at the footage's levels). */
typedef struct rvdd_resid_report {
    double ratio, ratio_lo, ratio_hi;   /* measured / predicted variance: all usable samples, their darkest and brightest third */
    double bias;                        /* mean residual, DN */
    double rho;                         /* correlation of horizontal same-plane neighbours */
    double a_fit, b_fit;                /* the curve the residual itself follows, DN */
    uint64_t samples;                   /* samples in the usable bins */
    int32_t bins;                       /* usable bins */
    int32_t reserved;                   /* 0 */
} rvdd_resid_report;
int rvdd_resid_fit(const rvdd_resid_acc* acc_host /* HOST copy */, int32_t bit_depth, double a, double b, rvdd_resid_report* out);

/* The measurement as a stage of rvdd_video_push: on != 0 switches it on, 0 off (the default).  Per handle; synchronises the device;
 * off -> on zeroes the accumulators.  With the stage on a push enqueues, right behind its frame-step and BEFORE rvdd_set_match's way
 * back, one rvdd_resid_stats launch per run of slots that gave an output (valid[b] = 1: heads and tails of option
 * "stream_all_frames" like any other; a slot without an output is not measured): the ring's centre frame -- as corrected by
 * rvdd_set_dpc_map / rvdd_set_dpc and as mapped by rvdd_set_match -- against out_rgb, into the slot's own accumulator
 * (cfg.batch x 3072 bytes on the device, allocated by the first push that has the stage on, freed with the handle), in the handle's
 * "bayer_pattern".  The unit: with rvdd_set_match on both sides are in the network's domain and bit_depth is 12, the unit of the
 * checkpoint's curve; with it off it is the push's bit_depth.  The stage only reads: out_rgb, valid and the recurrent state are bit
 * for bit those of the same pushes without it.  With the stage off a push makes exactly the launches it made before and allocates
 * nothing. */
int rvdd_set_resid(rvdd_t* h, int32_t on);

/* Slot `slot`'s accumulator copied to *host_out and zeroed on the device, both on `stream`, which is then synchronised: call it
 * where the loop synchronises anyway (the end of a video or of a shot).  All zeros on a handle that never pushed with the stage on.
 * RVDD_ERR_ARG: NULL host_out, slot outside 0 .. cfg.batch - 1. */
int rvdd_resid_read(rvdd_t* h, int32_t slot, rvdd_resid_acc* host_out /* HOST */, void* stream /* synchronised */);

/* ---- row noise (banding) ---------------------------------------------------------- */

/* The readout of a CMOS sensor adds to every sample of a mosaic row one offset that changes from row to row and from frame to frame:
 * horizontal banding that flickers.  It is common to the two colours of the mosaic row, so ONE offset is estimated per frame i, row
 * parity j (planes k = 2j and 2j + 1 of the packed [n,4,hh,ww] tensor, channel k = CFA position (k >> 1, k & 1)) and plane row r, from
 * the 2 ww samples of the row, and taken out of both planes.  Every operation is rounded to f32 on its own (no fused multiply-add):
 * offsets, states, counts and the corrected samples are reproducible bit for bit in NumPy f32 (tests/rows_ref.py).  With
 * top = (float)(2^bit_depth - 1), dn(v) = ((v + 1) * 0.5) * top and rvdd_dpc's way back 2 * (dn / top) - 1:
 *   per sample (k, r, c):
 *     x   = dn(p[k][r][c]); the eight vertical neighbours dn(p[k][r + dr][c]), dr in {+-1, +-2, +-3, +-4}, an index outside the plane
 *           mirrored about the site (r + dr -> r - dr: hence hh >= 5); where r - dr lies outside as well -- only in planes of fewer than
 *           nine rows -- it is reflected about the plane's edge (-q -> q, hh - 1 + q -> hh - 1 - q)
 *     m   = (s3 + s4) * 0.5, s3 / s4 the 4th / 5th of the eight in ascending order;  d = x - m
 *     var = fmaxf(noise_a * m - noise_b, var_floor)       the noise curve in DN of this bit depth
 *     the sample is USED iff d * d <= (k_gate * k_gate) * var      (edges, texture and defects fall outside the gate)
 *   per row (i, j, r):
 *     cnt = the used samples among the 2 ww.  The row is APPLIED iff cnt > 0 and 2 * cnt >= 2 * ww (integers: a row with exactly half
 *           of its samples used is applied), else SKIPPED with o = 0
 *     o   = (v[(cnt - 1) / 2] + v[cnt / 2]) * 0.5 of the used d in ascending order (d is never -0 under round-to-nearest: sorting by
 *           value is unambiguous), then clamped to [-max_dn, +max_dn]; the row is CLAMPED if the clamp changed it
 *   apply: in a row that is applied with o != 0 every sample of planes 2j and 2j + 1 becomes 2 * ((x - o) / top) - 1 (no clamp to the
 *     range); every other sample keeps its bits, and a frame in which no row has a non-zero offset is a bit copy.  gray [n,hh,ww]
 *     (nullable, patched IN PLACE): a gray row r in which at least one of the two parities has a non-zero offset is rewritten as
 *     (((d0 + d1) + d2) + d3) * 0.25 with d_k = dn(p[k][r][c]) - o[k >> 1][r]; every other gray row is not written.
 * What it cannot do: the median of eight vertical neighbours is itself shifted by THEIR rows' offsets, so about 0.4 of the offsets'
 * amplitude stays behind as a slow vertical drift that cannot be told from scene shading -- a limit of any single-frame rule without
 * optically black columns.  Rows that a long horizontal edge crosses are skipped, or biased by less than the gate.
 * Column fixed-pattern noise is the rule below (rvdd_cols_estimate), the gain between the two green planes the one after it
 * (rvdd_green_estimate); other offsets per plane and the use of the previous frame are out of scope.  Nothing is measured on real footage.
 * On footage WITHOUT row noise the estimate has an rms of about 1.35 sqrt(var / (2 ww)) of its own, which the stage then adds.
 *
 * rvdd_rows_estimate writes offsets (DEVICE float [n,2,hh]) and state (DEVICE uint8 [n,2,hh]: 0 skipped, 1 applied, 2 applied and
 * clamped), every word, and ADDS the rows of frame i to acc[i] (DEVICE, nullable, 8-byte aligned; integer atomics, the caller zeroes):
 * `applied` counts the rows of state 1 and 2, `clamped` those of state 2, sum_q2 is the sum of q * q with q = (int)rintf(o * 16), o as
 * written.  One workgroup per (frame, parity, row); the median of the used d is exact and takes the same steps whatever the values
 * (a digit-wise search of the keys' bit patterns: no histogram, no sorting of the row).  ww <= 4096.
 * rvdd_rows_apply takes the offsets out IN PLACE: a pure stream.  With ww % 4 == 0 and packed / gray 16-byte aligned a thread owns four
 * neighbouring cells (16-byte loads and stores), every other case one cell.  Same bits either way.
 * Inputs are assumed finite: with NaN or inf the result is unspecified, but nothing outside the tensors is read or written.
 * RVDD_ERR_ARG (the message names the argument) and nothing launched: NULL cfg; k_gate or max_dn not > 0 or not finite; noise_a /
 * noise_b not finite; var_floor not > 0 (or not finite); bit_depth outside 1..16; hh < 5; ww < 1 or > 4096; n < 0; NULL packed /
 * offsets / state with n > 0; acc not 8-byte aligned; a launch of more than 2^31 - 1 blocks.  n = 0 does nothing.  Asynchronous and
 * stream-ordered; nothing is read back. */
typedef struct rvdd_rows_cfg {
    float k_gate;             /* the gate in standard deviations of the noise curve, around 3 */
    float noise_a, noise_b;   /* var(m) = noise_a * m - noise_b, in DN of the frames' bit depth */
    float var_floor;          /* the least variance assumed, > 0 */
    float max_dn;             /* the largest offset taken out, in DN, > 0 */
} rvdd_rows_cfg;
typedef struct rvdd_rows_acc {   /* 24 bytes */
    uint32_t applied;         /* rows with an offset (state 1 or 2) */
    uint32_t skipped;         /* rows without (state 0) */
    uint32_t clamped;         /* rows whose offset met the clamp (state 2) */
    uint32_t reserved;        /* 0 */
    int64_t sum_q2;           /* sum of q * q, q = (int)rintf(o * 16): the rms offset is sqrt(sum_q2 / applied) / 16 DN */
} rvdd_rows_acc;
int rvdd_rows_estimate(rvdd_t* h, const float* packed /* [n,4,hh,ww] */, int32_t n, int32_t hh, int32_t ww, int32_t bit_depth,
                       const rvdd_rows_cfg* cfg, float* offsets /* DEVICE [n,2,hh] */, uint8_t* state /* DEVICE [n,2,hh] */,
                       rvdd_rows_acc* acc /* DEVICE [n], nullable, accumulated */, void* stream);
int rvdd_rows_apply(rvdd_t* h, float* packed /* [n,4,hh,ww], IN PLACE */, float* gray /* [n,hh,ww], nullable, in place */,
                    const float* offsets /* DEVICE [n,2,hh] */, int32_t n, int32_t hh, int32_t ww, int32_t bit_depth, void* stream);

/* The correction as a stage of rvdd_video_push: cfg = the parameters of rvdd_rows_estimate (checked as there: RVDD_ERR_ARG, the
 * message names the field, and nothing changes), NULL = off, the default.  Per handle; synchronises the device, as rvdd_set_dpc does;
 * off -> on zeroes the accumulators.  With the stage on a push runs, for every run of slots that got a frame, rvdd_rows_estimate and
 * rvdd_rows_apply on the ring's packed frames and gray planes IN PLACE with the push's bit_depth and cfg's curve -- the sensor's own,
 * in the DN of the footage -- behind rvdd_set_dpc_map and rvdd_set_dpc (defects are outliers that the gate drops anyway, but a
 * corrected sample counts) and in front of rvdd_set_match: two launches per run.  Everything downstream reads the ring, so the
 * corrected frames are what TV-L1 matches, what the step denoises, what rvdd_set_resid compares against and what option
 * "stream_all_frames" copies for a head or a tail, under every "stream_container".  The first push with the stage on allocates
 * offsets, states and one rvdd_rows_acc per slot (10 hh + 24 bytes per slot, freed with the handle); frames of hh < 5 or ww > 4096
 * cells are RVDD_ERR_ARG then.  With the stage off a push makes exactly the launches it made before and allocates nothing; a frame
 * whose offsets are all zero leaves the ring bit for bit what a push without the stage leaves. */
int rvdd_set_rows(rvdd_t* h, const rvdd_rows_cfg* cfg /* NULL = off, the default */);

/* Slot `slot`'s accumulator copied to *host_out and zeroed on the device, both on `stream`, which is then synchronised: call it where
 * the loop synchronises anyway (the end of a video or of a shot).  All zeros on a handle that never pushed with the stage on.
 * RVDD_ERR_ARG: NULL host_out, slot outside 0 .. cfg.batch - 1. */
int rvdd_rows_read(rvdd_t* h, int32_t slot, rvdd_rows_acc* host_out /* HOST */, void* stream /* synchronised */);

/* ---- column fixed-pattern noise ---------------------------------------------------- */

/* The other half of a CMOS readout: every mosaic column has its own amplifier or ADC offset, and that offset does NOT change from
 * frame to frame -- vertical stripes that stay put while the scene moves under them.  A mosaic column is shared by planes j and j + 2
 * of the packed [n,4,hh,ww] tensor (channel k = CFA position (k >> 1, k & 1); j = k & 1 is the column parity), so there is ONE offset
 * per column parity j and plane column c.  It is estimated per frame from the column's 2 hh samples (rvdd_cols_estimate, the transpose
 * of the row rule), pooled over F frames of a moving scene on the host (rvdd_cols_fit: the estimate's error falls as 1 / sqrt(F), scene
 * detail averages out, and a column is tested against its own spread before anything is changed), and taken out as a static map
 * (rvdd_cols_apply).  Every operation is rounded to f32 on its own (no fused multiply-add): offsets, states, the map and the corrected
 * samples are reproducible bit for bit in NumPy f32 (tests/cols_ref.py).  With top, dn(v) and the way back as for the rows:
 *   per sample (k, r, c):
 *     x   = dn(p[k][r][c]); the eight horizontal neighbours dn(p[k][r][c + dc]), dc in {+-1, +-2, +-3, +-4}, an index outside the plane
 *           mirrored about the site (c + dc -> c - dc: hence ww >= 5); where c - dc lies outside as well -- only in planes of fewer than
 *           nine columns -- it is reflected about the plane's edge (-q -> q, ww - 1 + q -> ww - 1 - q)
 *     m   = (s3 + s4) * 0.5, s3 / s4 the 4th / 5th of the eight in ascending order;  d = x - m
 *     var = fmaxf(noise_a * m - noise_b, var_floor)       the noise curve in DN of this bit depth
 *     the sample is USED iff d * d <= (k_gate * k_gate) * var
 *   per frame and column (i, j, c):
 *     cnt = the used samples among the 2 hh.  The column is APPLIED (state 1) iff cnt > 0 and cnt >= hh, with
 *     e   = (v[(cnt - 1) / 2] + v[cnt / 2]) * 0.5 of the used d in ascending order (the exact median); else SKIPPED (state 0), e = 0.
 *           There is no clamp here.
 *   the fit over F frames (rvdd_cols_fit, on the host, f32, in this order), for each (j, c):
 *     v   = the e of the frames with state 1, ascending; nf = how many there are.  nf < max(1, min_frames): map = 0, mstate 0
 *           (UNSUPPORTED).  Otherwise
 *     o   = (v[(nf - 1) / 2] + v[nf / 2]) * 0.5;  a[i] = |v[i] - o|, ascending;  mad = (a[(nf - 1) / 2] + a[nf / 2]) * 0.5
 *     (o * o) * (float)nf < (k_sig * k_sig) * (3.4528f * (mad * mad)): map = 0, mstate 3 (INSIGNIFICANT).  3.4528 = (1.4826 * 1.2533)^2
 *           is the variance of a median in units of MAD^2; k_sig = 0 keeps every supported column.  Otherwise
 *     map = o clamped to [-max_dn, +max_dn], mstate 1 (APPLIED), or 2 if the clamp changed it (CLAMPED).
 *   apply (map [2,ww] f32 in DN of the frames' bit depth, in place, a pure stream): where map[k & 1][c] != 0 the sample becomes
 *     2 * ((x - map) / top) - 1 (no clamp to the range); every other sample keeps its bits.  gray [n,hh,ww] (nullable): a gray cell in a
 *     column c where at least one parity's map is non-zero is rewritten as (((d0 + d1) + d2) + d3) * 0.25, d_k = dn(p[k][r][c]) -
 *     map[k & 1][c]; every other gray cell is not written.  A map of zeros leaves the tensors bit for bit.
 * What it cannot do: the neighbours carry offsets too, so the estimate is a high-pass of the pattern -- slow horizontal shading of the
 * pattern stays, as for the rows.  In a tripod shot of a static scene a vertical edge passes the significance test, because its spread
 * over time is only noise: estimate on footage that moves.  One camera setting per map.  The gain between the two green planes is the next rule
 * (rvdd_green_estimate); other offsets per plane and per-column gains are out of scope.  Nothing is measured on real footage.
 *
 * rvdd_cols_estimate writes offsets (DEVICE float [n,2,ww]) and state (DEVICE uint8 [n,2,ww]: 0 skipped, 1 applied), every word.  One
 * workgroup per (frame, parity, strip of 32 / 16 / 8 / 4 neighbouring columns for hh <= 639 / 1279 / 2559 / 4096): the strip's keys lie
 * column-major in LDS, one wave finds a column's exact median by a digit-wise search of the keys' bit patterns that takes the same
 * steps whatever the values.  hh <= 4096: four columns of 2 hh 32-bit keys are what fits the 160 KiB of a CU with a wave's count
 * below 2^16.  Inputs are assumed finite.  RVDD_ERR_ARG (the message names the argument) and nothing launched: NULL cfg; k_gate not
 * > 0 or not finite; noise_a / noise_b not finite; var_floor not > 0 (or not finite); bit_depth outside 1..16; ww < 5; hh < 1 or
 * > 4096; n < 0; NULL packed / offsets / state with n > 0; a launch of more than 2^31 - 1 blocks.  n = 0 does nothing.  Asynchronous
 * and stream-ordered; nothing is read back.
 * rvdd_cols_fit needs no device and no handle (errors: rvdd_last_error(NULL)).  stats (nullable): counts[s] = the columns of mstate s,
 * sum_q2 = the sum of q * q with q = (int)rintf(16 * map), floor_dn = the mean over the supported columns (mstate 1, 2, 3) of
 * ((1.2533f * 1.4826f) * mad) / sqrtf(nf), summed in f64 in the order (j, c): the standard error of the pooled estimate.
 * RVDD_ERR_ARG: a NULL pointer but stats; F < 1; ww < 1; k_sig < 0 or not finite; max_dn not > 0 or not finite.
 * rvdd_cols_apply takes map_dev (DEVICE [2,ww]) out IN PLACE.  With ww % 4 == 0 and packed / gray / map_dev 16-byte aligned a thread
 * owns four neighbouring cells (16-byte loads and stores), every other case one cell.  Same bits either way.  RVDD_ERR_ARG as for the
 * estimate's shape (hh has no cap here), NULL packed / map_dev with n > 0. */
typedef struct rvdd_cols_cfg {
    float k_gate;             /* the gate in standard deviations of the noise curve, around 3 */
    float noise_a, noise_b;   /* var(m) = noise_a * m - noise_b, in DN of the frames' bit depth */
    float var_floor;          /* the least variance assumed, > 0 */
} rvdd_cols_cfg;
typedef struct rvdd_cols_fit_cfg {
    int32_t min_frames;       /* the least number of applied frames a column needs; below 1 counts as 1 */
    float k_sig;              /* the significance threshold in standard errors of the pooled median, >= 0; 0 keeps every supported column */
    float max_dn;             /* the largest offset taken out, in DN, > 0 */
} rvdd_cols_fit_cfg;
typedef struct rvdd_cols_stats {   /* 32 bytes */
    uint32_t counts[4];       /* columns by mstate: 0 unsupported, 1 applied, 2 applied and clamped, 3 insignificant */
    int64_t sum_q2;           /* sum of q * q, q = (int)rintf(16 * map): the map's rms is sqrt(sum_q2 / (2 ww)) / 16 DN */
    double floor_dn;          /* the mean standard error of the pooled estimates, in DN */
} rvdd_cols_stats;
int rvdd_cols_estimate(rvdd_t* h, const float* packed /* [n,4,hh,ww] */, int32_t n, int32_t hh, int32_t ww, int32_t bit_depth,
                       const rvdd_cols_cfg* cfg, float* offsets /* DEVICE [n,2,ww] */, uint8_t* state /* DEVICE [n,2,ww] */, void* stream);
int rvdd_cols_fit(const float* offsets_host /* [F,2,ww] */, const uint8_t* state_host /* [F,2,ww] */, int32_t F, int32_t ww,
                  const rvdd_cols_fit_cfg* fit_cfg, float* map_host /* [2,ww] */, uint8_t* mstate_host /* [2,ww] */,
                  rvdd_cols_stats* stats_host /* nullable */);
int rvdd_cols_apply(rvdd_t* h, float* packed /* [n,4,hh,ww], IN PLACE */, float* gray /* [n,hh,ww], nullable, in place */,
                    const float* map_dev /* DEVICE [2,ww] */, int32_t n, int32_t hh, int32_t ww, int32_t bit_depth, void* stream);

/* The map as a stage of rvdd_video_push: map_host [2,ww] f32 in DN of the pushes' bit depth (every value finite, ww >= 5: else
 * RVDD_ERR_ARG and nothing changes), NULL = off, the default.  Per handle; synchronises the device as rvdd_set_dpc_map does, copies
 * the map to the device (8 ww bytes, freed by the next call and with the handle).  With the stage on a push runs, for every run of
 * slots that got a frame, ONE rvdd_cols_apply on the ring's packed frames and gray planes IN PLACE, behind rvdd_set_dpc_map and
 * rvdd_set_dpc and in front of rvdd_set_rows and rvdd_set_match; a push of frames with another ww is RVDD_ERR_ARG.  The map is static:
 * no per-slot state and no read call.  With the stage off a push makes exactly the launches it made before and allocates nothing; a
 * map of zeros leaves the ring bit for bit what a push without the stage leaves. */
int rvdd_set_cols(rvdd_t* h, const float* map_host /* [2,ww]; NULL = off, the default */, int32_t ww);

/* ---- green imbalance ------------------------------------------------------------------ */

/* The green sites of the red rows (Gr) and of the blue rows (Gb) see the same light through different neighbours, and pixel crosstalk
 * makes their responses differ by up to a few per cent of the signal: a gain that varies slowly over the field with the ray angle
 * and is static for one camera, lens and aperture.  Hamilton-Adams interpolates green at a red or blue site from two sites of either
 * kind and picks the direction by gradients, so an imbalance below the noise becomes a maze pattern.  The gain is estimated per frame
 * and block (rvdd_green_estimate), pooled over F frames on the host with a significance test (rvdd_green_fit) and taken out as a
 * static map (rvdd_green_apply).  Every operation is rounded to f32 on its own (no fused multiply-add): e, level, states, the map and
 * the corrected samples are reproducible bit for bit in NumPy f32 (tests/green_ref.py).
 *   planes and geometry: packed [n,4,hh,ww], plane k = CFA position (k >> 1, k & 1).  Under GBRG / GRBG the greens are planes 0 and 3,
 *     under RGGB / BGGR planes 1 and 2.  A = the green plane of CFA row 0, B = that of CFA row 1; dx = -1 where A sits in CFA column
 *     0, +1 where it sits in column 1.  top, dn(v) and the way back are as for the rows.
 *   per sample, two sides:
 *     A-side: a cell (r, c) is an A-side sample iff the four B cells (r + {0, -1}, c + {0, dx}) lie in the plane -- the B sites
 *       diagonally next to A(r, c) on the mosaic.  B-side: iff the four A cells (r + {0, +1}, c + {0, -dx}) lie in the plane.  Cells
 *       that are not samples do not count anywhere.
 *     x   = the sample's DN;  m = (s1 + s2) * 0.5, s1 / s2 the 2nd / 3rd of the four neighbours in ascending order;  d = x - m
 *     var = fmaxf(noise_a * m - noise_b, var_floor);  the sample is USED iff d * d <= (k_gate * k_gate) * var.  The four neighbours are
 *       symmetric about the site, so a planar scene gradient cancels in d.
 *   per frame and block of RVDD_GREEN_BLOCK x RVDD_GREEN_BLOCK = 32 x 32 cells (gh = ceil(hh / 32), gw = ceil(ww / 32); the last
 *   blocks are partial):
 *     tot_A, tot_B = the block's samples of each side, cnt_A, cnt_B = the used ones.  The block is APPLIED (state 1) iff cnt_A > 0,
 *       cnt_B > 0, 2 cnt_A >= tot_A and 2 cnt_B >= tot_B.  Then
 *     e     = (med_A - med_B) * 0.5, med the exact median (v[(cnt - 1) / 2] + v[cnt / 2]) * 0.5 of the side's used d.  The scene's
 *       curvature enters both sides with the same sign and cancels; the imbalance enters with opposite signs and stays.
 *     level = (float)((double)S / (double)(cnt_A + cnt_B)), S the 64-bit integer sum of (int)rintf(m) over the used samples of both
 *       sides.  Else the block is SKIPPED (state 0) with e = level = 0.
 *   the fit over F frames (rvdd_green_fit, on the host, f32, in this order), per block:
 *     v   = q = e / (level - black) of the frames with state 1 and level - black >= min_signal, ascending; nf of them.  Then exactly
 *       rvdd_cols_fit's pooled step: nf < max(1, min_frames): map = 0, mstate 0.  o = the median, mad = the median of |v - o|.
 *       o == 0, or (o * o) * (float)nf < (k_sig * k_sig) * (3.4528f * (mad * mad)): map = 0, mstate 3.  Else map = o clamped to
 *       [-max_gain, +max_gain], mstate 1, or 2 if the clamp changed it.
 *     stats: counts by mstate; sum_q2 with q = (int)rintf(16384 * map); floor = the mean over the supported blocks (mstate 1, 2, 3) of
 *       ((1.2533f * 1.4826f) * mad) / sqrtf(nf), summed in f64 in block order; the FLAT estimate: the same pooled step (at least one
 *       value) over the o of the supported blocks, in block order, in the frames' place: flat_gain, flat_se, flat_state.
 *   apply (map [gh,gw] f32 gains of A relative to B -- the frame's own grid, or [1,1] for a flat gain --, in place, a pure stream), per
 *   cell (r, c):
 *     fy = ((float)r + 0.5f) * (1 / 32) - 0.5f clamped to [0, gh - 1];  y0 = (int)fy, y1 = min(y0 + 1, gh - 1), wy = fy - (float)y0;
 *       likewise fx, x0, x1, wx from c and gw.
 *     t = g[y0][x0] + wx * (g[y0][x1] - g[y0][x0]);  u likewise on row y1;  g = t + wy * (u - t);  h = 0.5f * g.
 *     where g != 0: A's sample becomes x - h * (x - black), B's x + h * (x - black), packed again as 2 * (dn / top) - 1 with no clamp
 *       to the range, and the gray cell (gray [n,hh,ww], nullable) is rewritten as (((d0 + d1) + d2) + d3) * 0.25 with the corrected
 *       DN.  Where g == 0 the four samples keep their bits and the gray cell is not written.  The two planes that are not green are
 *       never written.  A map of zeros leaves the tensors bit for bit.
 * What it cannot do: the gate is centred on zero, so an imbalance of delta shrinks by about phi(k) / phi(0) of itself on the way in
 * (a throw-away f64 prototype of this rule recovered 0.93 - 0.95 of an injected 1 - 5 %).  e is a MEDIAN of differences and level a MEAN:
 * where the signal varies several-fold inside a block and is dark-heavy, the median lies below the mean and less comes back (0.63 -
 * 0.72 on the synthetic sequences of DESIGN.md 4.22).  Texture finer than two cells aliases into
 * d.  One camera, lens and aperture per map.  Nothing is measured on real footage.
 *
 * rvdd_green_estimate writes e, level (DEVICE float [n,gh,gw]) and state (DEVICE uint8 [n,gh,gw]: 0 skipped, 1 applied), every word,
 * skipped blocks included, and only reads packed.  One workgroup per (frame, block): the block's two green planes go to LDS once with
 * their one-cell halo, the two medians are exact (the digit-wise search of the rows and columns).  Inputs are assumed finite.
 * RVDD_ERR_ARG (the message names the argument) and nothing launched: NULL cfg; k_gate or var_floor not > 0 or not finite; noise_a /
 * noise_b / black not finite; bit_depth outside 1..16; pattern outside enum rvdd_bayer; hh < 2 or ww < 2; n < 0; NULL packed / e /
 * level / state with n > 0; more than 2^31 - 1 blocks.  n = 0 does nothing.  Asynchronous and stream-ordered; nothing is read back.
 * cfg.black is not read by the estimate: it travels with the rule to the fit and the apply.
 * rvdd_green_fit needs no device and no handle (errors: rvdd_last_error(NULL)).  RVDD_ERR_ARG: a NULL pointer but stats; F, gh or gw
 * < 1; black not finite; k_sig < 0 or not finite; max_gain or min_signal not > 0 or not finite.
 * rvdd_green_apply takes map_dev (DEVICE [gh,gw]) out IN PLACE.  With ww % 4 == 0 and packed / gray 16-byte aligned a thread owns
 * four neighbouring cells (16-byte loads and stores), every other case one cell.  Same bits either way.  RVDD_ERR_ARG as for the
 * estimate's shape and pattern; NULL packed / map_dev with n > 0; black not finite; a grid (gh, gw) that is neither [1,1] nor the
 * frame's own. */
#define RVDD_GREEN_BLOCK 32
typedef struct rvdd_green_cfg {
    float k_gate;             /* the gate in standard deviations of the noise curve, around 3 */
    float noise_a, noise_b;   /* var(m) = noise_a * m - noise_b, in DN of the frames' bit depth */
    float var_floor;          /* the least variance assumed, > 0 */
    float black;              /* the level without signal, in DN: noise_b / noise_a where the curve's variance is zero there */
} rvdd_green_cfg;
typedef struct rvdd_green_fit_cfg {
    int32_t min_frames;       /* the least number of usable frames a block needs; below 1 counts as 1 */
    float k_sig;              /* the significance threshold in standard errors of the pooled median, >= 0 */
    float max_gain;           /* the largest gain taken out, > 0 (0.10 = 10 %) */
    float min_signal;         /* the least level - black, in DN, at which a frame's block counts, > 0 */
} rvdd_green_fit_cfg;
typedef struct rvdd_green_stats {   /* 48 bytes */
    uint32_t counts[4];       /* blocks by mstate: 0 unsupported, 1 applied, 2 applied and clamped, 3 insignificant */
    int64_t sum_q2;           /* sum of q * q, q = (int)rintf(16384 * map): the map's rms gain is sqrt(sum_q2 / (gh gw)) / 16384 */
    double floor;             /* the mean standard error of the pooled estimates, as a gain */
    float flat_gain;          /* the flat estimate: the pooled median of the supported blocks' medians, clamped; 0 unless flat_state is 1 or 2 */
    float flat_se;            /* its standard error */
    int32_t flat_state;       /* its mstate */
    int32_t reserved;         /* 0 */
} rvdd_green_stats;
int rvdd_green_estimate(rvdd_t* h, const float* packed /* [n,4,hh,ww] */, int32_t n, int32_t hh, int32_t ww, int32_t bit_depth,
                        int32_t pattern /* enum rvdd_bayer */, const rvdd_green_cfg* cfg, float* e /* DEVICE [n,gh,gw] */,
                        float* level /* DEVICE [n,gh,gw] */, uint8_t* state /* DEVICE [n,gh,gw] */, void* stream);
int rvdd_green_fit(const float* e_host /* [F,gh,gw] */, const float* level_host /* [F,gh,gw] */, const uint8_t* state_host /* [F,gh,gw] */,
                   int32_t F, int32_t gh, int32_t gw, float black, const rvdd_green_fit_cfg* fit_cfg, float* map_host /* [gh,gw] */,
                   uint8_t* mstate_host /* [gh,gw] */, rvdd_green_stats* stats_host /* nullable */);
int rvdd_green_apply(rvdd_t* h, float* packed /* [n,4,hh,ww], IN PLACE */, float* gray /* [n,hh,ww], nullable, in place */,
                     const float* map_dev /* DEVICE [gh,gw] */, int32_t gh, int32_t gw, float black, int32_t n, int32_t hh, int32_t ww,
                     int32_t bit_depth, int32_t pattern /* enum rvdd_bayer */, void* stream);

/* The map as a stage of rvdd_video_push: map_host [gh,gw] f32 gains (every value finite, gh and gw >= 1, black finite: else
 * RVDD_ERR_ARG and nothing changes), NULL = off, the default.  Per handle; synchronises the device and copies the map, as
 * rvdd_set_cols does (4 gh gw bytes, freed by the next call and with the handle).  With the stage on a push runs, for every run of
 * slots that got a frame, ONE rvdd_green_apply on the ring's packed frames and gray planes IN PLACE under the handle's option
 * "bayer_pattern", behind rvdd_set_dpc_map, rvdd_set_dpc, rvdd_set_cols and rvdd_set_rows -- readout offsets come off before a pixel
 * gain is judged -- and in front of rvdd_set_match.  A push whose frames have another grid than a map that is not [1,1] is
 * RVDD_ERR_ARG, as is one of frames with hh < 2 or ww < 2.  The map is static: no per-slot state and no read call.  With the stage off
 * a push makes exactly the launches it made before and allocates nothing; a map of zeros leaves the ring bit for bit what a push
 * without the stage leaves. */
int rvdd_set_green(rvdd_t* h, const float* map_host /* [gh,gw]; NULL = off, the default */, int32_t gh, int32_t gw, float black);

/* ---- raw datasets from sRGB video ------------------------------------------- */

/* dataset/generate_raw_from_RGB.py (:45-127 single_image_rgb2raw, :168-189 the 12-bit range, the percentile matching to CRVD
 * and the noise) in one pointwise kernel: sRGB frames -> the four images the reference writes per frame, all HWC.
 * Per pixel and channel, every operation rounded to f32 on its own and both divisions correctly rounded:
 *   v   = clamp(((float)srgb + dither) / 266, 0, 1)
 *   p   = pow(max(0.5 - sin(asin(1 - 2 v) / 3), 1e-8), 2.2)                 inverse smoothstep, gamma expansion
 *   cam[k] = (p[0] M[k][0] + p[1] M[k][1]) + p[2] M[k][2]                   the CRVD rgb2cam matrix (:101)
 *   y   = clamp(cam[k] * g[k], 0, 1),  g = ((1 / red_gain) / rgb_gain, 1 / rgb_gain, (1 / blue_gain) / rgb_gain) formed in
 *         f32 on the host from the gains rounded to f32 (:77)
 *   lin = y * 3855 + 240;  lin = A * (lin - 245) / 2060 + B,  (A, B) = (3344, 266) at ISO 3200, (3807, 268) at ISO 12800
 * Outputs (each may be NULL; with all four NULL nothing is launched):
 *   lin_f32 [n,H,W,3]      lin -- what rvdd_ppipe(bit_depth 12, HWC strides) takes to make gt_RGB;
 *   lin_u16 [n,H,W,3]      clip(rint(lin), 0, 4095): gt_raw_linear_RGB;
 *   gt_raw  [n,H/2,W/2,4]  the mosaic of lin in `pattern` (enum rvdd_bayer; GBRG is the reference's mosaic()): channel k is
 *                          CFA position (k >> 1, k & 1) of a 2x2 cell -- RVDD_RAW_PACKED_HWC in f32, which rvdd_ingest_raw and
 *                          rvdd_video_push read as it lies;
 *   noisy   [n,H/2,W/2,4]  m + sqrt(max(ka * m - kb, 0)) * z of the mosaic m: (ka, kb) = (8.0034, 2043.51144) at ISO 3200,
 *                          (28.3015, 6307.62081) at ISO 12800.
 * The draws.  dither [n,H,W,3] (the reference's uniform quantisation noise in [-0.5, 0.5)) and normal [n,H/2,W/2,4] (z) may be
 * handed in; where one is NULL the kernel draws it with Philox4x32-10 (multipliers 0xD2511F53 / 0xCD9E8D57, key increments
 * 0x9E3779B9 / 0xBB67AE85): key = (low, high) 32 bits of `seed`, counter = (element, stream, low, high 32 bits of frame0 + i)
 * for image i of the call, output words w_0..w_3.
 *   stream 0, element = pixel y * W + x: dither of channel c = (w_c >> 8) * 2^-24 - 0.5 (exact in f32);
 *   stream 1, element = cell y * (W/2) + x: u = ((w_0 >> 8) + 1) * 2^-24, v = (w_1 >> 8) * 2^-24, r = sqrt(-2 ln u),
 *             (z_0, z_1) = (r cos 2 pi v, r sin 2 pi v), (z_2, z_3) the same from (w_2, w_3); z_k goes to CFA position k.
 * The 24-bit uniforms end the normal's tail at sqrt(48 ln 2) = 5.77 sigma.  A draw depends on (seed, frame, element) alone, so:
 *   - rvdd_unprocess with NULL planes is bit for bit rvdd_unprocess fed the planes rvdd_unprocess_draws writes for the same
 *     (seed, frame0, n, H, W);
 *   - a call of n frames is bit for bit n calls of one frame at frame0 + i.
 * iso other than 3200 / 12800, odd H or W, pattern outside 0..3, H * W >= 2^32, n < 0 or a zero gain: RVDD_ERR_ARG (the message
 * names the argument).  n = 0 does nothing.  Asynchronous and stream-ordered; nothing is read back.  With (W/2) % 4 == 0 and
 * 16-byte aligned pointers a thread takes two cells with 16-byte stores; same bits either way. */
int rvdd_unprocess(rvdd_t* h, const uint8_t* srgb /* [n,H,W,3] */, int32_t n, int32_t H, int32_t W,
                   double rgb_gain, double red_gain, double blue_gain, int32_t iso, int32_t pattern /* enum rvdd_bayer */,
                   const float* dither /* nullable */, const float* normal /* nullable */, uint64_t seed, int64_t frame0,
                   float* lin_f32, uint16_t* lin_u16, float* gt_raw, float* noisy, void* stream);

/* The two planes rvdd_unprocess draws for (seed, frame0 .. frame0 + n - 1), alone: dither [n,H,W,3], normal [n,H/2,W/2,4];
 * either may be NULL.  Shape errors as rvdd_unprocess.  Asynchronous and stream-ordered. */
int rvdd_unprocess_draws(rvdd_t* h, uint64_t seed, int64_t frame0, int32_t n, int32_t H, int32_t W,
                         float* dither, float* normal, void* stream);

/* dataset/fwd_ppipe.py `ppipe(im, rgb_gain, red_gain, blue_gain, iso)` (:48-77) fused with the range
 * normalisation in front of it (:131-137) and the uint8 conversion behind it (:141): linear camera RGB ->
 * display sRGB (inverse percentile matching per ISO, black level, white-balance gains, inverse CCM,
 * gamma 1/2.2, smoothstep tone curve, x255).
 *   img        n images of 3 channels, element (i,c,y,x) at img[i*stride_n + c*stride_c + y*stride_y + x*stride_x]
 *              (NCHW network output or the HWC image validate.py writes -- both are strides);
 *   bit_depth  fwd_ppipe.py --bit_depth: 0 ([0,1]), 8 ([0,255]), 10, anything else = already [0,4095];
 *              RVDD_PPIPE_FROM_NET (-1) = network output in [-1,1]: util/util.py:40 (tensor2im) then the 8-bit branch;
 *   gains      the three values fwd_ppipe.py:116-118 passes (rgb_gain = 1/n from the white-balance table);
 *   out_u8     [n,H,W,3] uint8 (what the reference writes to *_processed_pipeline.png);
 *   out_f32    [n,H,W,3] float32 = ppipe()'s return value before rounding; may be NULL. */
#define RVDD_PPIPE_FROM_NET (-1)
int rvdd_ppipe(rvdd_t* h, const float* img, int32_t n, int32_t height, int32_t width, int64_t stride_n,
               int64_t stride_c, int64_t stride_y, int64_t stride_x, int32_t bit_depth, double rgb_gain,
               double red_gain, double blue_gain, int32_t iso, uint8_t* out_u8, float* out_f32, void* stream);

/* Display images as frames of a Y'CbCr 4:2:0 video: BT.709, limited range, chroma a box average of each 2 x 2 quad (centre-sited,
 * the `420jpeg` siting of Y4M), 8 or 10 bits.  Integer after ONE quantisation, so that it is held bit for bit (tests/ycbcr_ref.py):
 *   disp     [n,H,W,3] float32 display values d nominally in [0,255] -- what rvdd_ppipe writes to out_f32; H, W even;
 *   depth    D = 8 or 10; m = 2^(D-8); K = 65535 * 16384;
 *   q_c      = (int) rintf(min(max(d_c, 0), 255) * 257.0f) in 0 .. 65535: one f32 product, rounded half to even; a NaN gives 0;
 *   luma, per pixel:      L  = 3483 q_r + 11718 q_g + 1183 q_b (the coefficients sum to 16384),
 *                         Y  = 16 m + floor((L * 219 m + K / 2) / K);
 *   chroma, per 2 x 2 quad, s_c = the sum of its four q_c:
 *                         cb = -1877 s_r - 6315 s_g + 8192 s_b,   cr = 8192 s_r - 7441 s_g - 751 s_b (each row sums to 0),
 *                         Cb = 128 m + floor((cb * 224 m + 2 K) / (4 K)), Cr likewise: floor division of a signed 64-bit numerator;
 *   frames   [n, H*W*3/2] samples, uint8 (D = 8) or little-endian uint16 (D = 10): per image one Y4M frame body, the Y plane
 *            [H,W], then Cb, then Cr, [H/2,W/2] each.
 * White is 235 m, black 16 m, any grey has Cb = Cr = 128 m, pure blue Cb = 240 m, exactly; against the real-valued BT.709 formula
 * every sample lies within 0.5 + 0.09 codes (three 14-bit coefficient roundings, 3 * 2^-15 * 876 = 0.08, and the 16-bit input
 * quantisation, 0.007).  n = 0 does nothing and accepts NULL pointers.  RVDD_ERR_ARG, the argument named: odd or non-positive H
 * or W, a depth other than 8 or 10, n < 0, a NULL disp or frames with n > 0, a launch of more than 2^31 - 1 blocks.
 * Asynchronous and stream-ordered; reads nothing back. */
int rvdd_ycbcr(rvdd_t* h, const float* disp /* [n,H,W,3] */, int32_t n, int32_t H, int32_t W, int32_t depth /* 8 | 10 */,
               void* frames /* [n, H*W*3/2] uint8 | uint16 */, void* stream);

/* dataset/fwd_ppipe.py `psnr(img1, img2)` (:79-84) and `ssim` (:86, skimage.metrics.structural_similarity with
 * multichannel=True, data_range=255: 7x7 uniform window, sample covariance, 3-pixel border cropped) on uint8
 * [n,H,W,3] images.  psnr / ssim: HOST arrays of n doubles (either may be NULL).  H, W >= 7.  Synchronous. */
int rvdd_srgb_metrics(rvdd_t* h, const uint8_t* a, const uint8_t* b, int32_t n, int32_t height, int32_t width,
                      double* psnr, double* ssim, void* stream);

/* Options of recurrentModel that change what a step does (models/recurrent_model.py:27-36).  Known names:
 *   "no_warp"  (--no_warp, :137-159): the previous output, the previous features and the next frame enter the net
 *              unwarped; rvdd_step then ignores flow_prev / flow_next (they may be NULL).
 *   "warp_raw" (--warp_raw, :149-152): the previous output is re-mosaicked, warped at RAW resolution with the
 *              raw-resolution flow and demosaicked again (the next frame: warped as packed raw, then demosaicked).
 *              Not defined with feature recurrence (the reference fails on the shapes there): error.
 *   "prev_noisy_frame" (--prev_noisy_frame, :33, :335-337): the frame handed to the next step as "previous" is the
 *              demosaiced NOISY current frame, not the denoised one (the feature recurrence is unaffected).
 *   "conv_kernel": which kernel runs the convunet's 3x3 convs.  0 (default) = EVERY 3x3 conv of the net -- the
 *              16-channel first layer and UpConv's fused upsample included -- on the F16 matrix pipe with each f32
 *              operand split into two f16 halves, three MFMAs per product, f32 accumulation (conv3x3h.hip: as close
 *              to the reference as the f32 kernels).  The f16 exponent range is not a limit
 *              of the path: every map carries its max |x| per sequence and is multiplied by a power of two before
 *              the split (block floating point, exact), so frames of any finite magnitude keep fp32 semantics
 *              (tests/test_gpu_parity.py::test_split_path_any_magnitude).  1 = the direct f32 kernel everywhere;
 *              2 = the Winograd f32 kernel everywhere; 4 = f32 kernels chosen by launch size (1, 2, 4: exact-f32
 *              products, the A/B reference, about 0.7 of the default's frame rate at 720p).
 *   "seq_major": 1 = the full-resolution stages of the convunet run one sequence at a time (measured slower; off).
 *   "fuse_upsample": 0 = UpConv's bilinear x2 upsample runs as its own kernel instead of inside the Winograd patch
 *              load of the conv behind it (default 1; same bits either way).
 *   "graphs":   1 = frame-steps are captured into hipGraphs and replayed (measured slower on ROCm 7.2; off).
 *   "next_split": 0 = ConvNeXtUnet's ConvBlock (networks/new_unet.py:74-103, one fused kernel) multiplies its two 1x1 convs on the f32 matrix pipe (exact-f32 products) instead
 *               of the F16 pipe with split f32 operands (the default, as "conv_kernel" 0; the A/B reference).  The split
 *               operands are bounded by the block's LayerNorm whatever the frames are; a block whose weights would let
 *               them leave the f16 range (checked at rvdd_finalize_weights) runs the f32 form by itself.
 *   "next_pipe": 0 = the fused ConvBlock runs its three phases one after the other in all eight waves of a workgroup
 *               (convblock_kernel) instead of as a pipeline over tiles -- depth-wise conv and LayerNorm of the next tile on
 *               four waves beside the MLP of the current one on the other four (convblock_pipe_kernel, the default with
 *               next_split; same bits either way).
 *   "next_pool": 0 = MaxPool2d(2) in front of a DownConv (new_unet.py:200-204) as its own kernel instead
 *               of the fused block's epilogue (default 1; same bits either way).
 *   "cout_split": 0 = every launch of the split-f16 conv kernel forms all 48 output channels of a tile in one workgroup.
 *               Default 1: a launch with at most a third of a 16x16 tile per compute unit (the coarse levels of one small
 *               sequence) gives a tile to three workgroups of 16 output channels each -- a third of the filter bank's copy and
 *               of the matrix work per workgroup; same sums in the same order, same bits.  Per handle.
 *   "small_prestage": 0 = the pre-stage of a frame-step (bound of the network input, green plane, network input) always as
 *               its three kernels.  Default 1: a step of at most 1024 tiles of 16x16 pixels without a future frame (a single
 *               small sequence: the launches there are 5-15 us each, back to back) forms them in one kernel; a larger step
 *               without a future frame forms the network input in that kernel too, tile by tile with the green plane in
 *               on-chip memory, behind the bound's own small launch; same bits.  Per handle.
 *   "warp48_pairs": 1 = the bicubic warp of the 48 recurrent feature channels (warp48_kernel) shares its loads within
 *               horizontally adjacent pixel pairs only (20 loads for two pixels whose 4x4 footprints line up).  Default 0: the
 *               four pixels of a 2x2 quad whose footprints are the same five rows and columns share 25 loads; quads that do not
 *               line up fall back to the pair form row by row.  The same values, weights and order of sums per pixel: same bits
 *               (the A/B reference).  Inert where the warp carries ConvNeXtUnet's projection (warp48_proj_kernel: pairs
 *               always).  Per handle.
 *   "tvl1_async": 1 = rvdd_tvl1flow_batch called without iteration counts enqueues its launches on the stream and returns
 *               (the flows are ready in stream order; nothing is read back, the stream is not synchronised): the form for a
 *               caller that feeds the flows straight into rvdd_step on the same stream (validate.py's --val_flow_from_denoised loop
 *               on the device).  The batch's control word -- set only if a grid barrier of the TV-L1 kernels gave up -- is then
 *               read by the next call that synchronises anyway: rvdd_psnr_l1, a TV-L1 call that returns iteration counts or runs
 *               with the option off, or this option set back to 0 (each reports RVDD_ERR_HIP then).  Default 0: the reference
 *               bridge's behaviour (library.py:150-175 returns finished host arrays).
 *   "next_projfuse": 0 = the 96 -> 48 projection of the ConvBlock behind a concat (new_unet.py:85-88, 321-329) as its own
 *               kernel, instead of as two 48 -> 48 halves in the epilogues of the blocks that form the two concatenated maps
 *               (default 1 with the pipelined split-f16 block; the A/B reference: the same linear map, summed in another
 *               order).
 *   "fuse_pre": 0 = preprocessing_layer (3x3, no activation, networks/unet.py:742) and the first source of EncoderConvs[0][0]
 *               (3x3, :743) run as the two convs they are, instead of as their composition -- ONE 5x5 conv of the network
 *               input plus a fix of the border ring, where the zero padding between the two layers matters (default 1, the
 *               feature-recurrent convunet on the split-f16 path; the A/B reference: the same linear map, summed in another
 *               order, a few 1e-7 apart).
 *   "pre5_cin8": 0 = the composed first layer ("fuse_pre") multiplies all 16 channels of the network input's pixel, 25 taps x 2
 *               eight-channel groups = 13 chunks of K, also where at most 8 of them are real.  Default 1: a network without a
 *               future frame (6 real channels) multiplies the first eight only, 25 groups = 7 chunks -- the other group of every
 *               tap is zero filters on zero input; half the halo loads, splits and staging stores as well.  The same linear map
 *               with K grouped differently (a few 1e-6 apart).  Inert with a future frame (9 channels).  Per handle.
 *   "block_fp": 0 = the split-f16 convs split their operands without the per-map power of two (the A/B reference of the block
 *               floating point; right only while every activation stays within 2^-14 .. 65504).  Default 1.
 *   "bayer_pattern": enum rvdd_bayer of the packed raw frames rvdd_step is handed (--bayer_pattern): every demosaic and
 *               re-mosaic of a step follows it -- the current and next frames, raw_prev on a first step and on
 *               rvdd_reset_slots, --prev_noisy_frame and --warp_raw.  Default 0 (GBRG); any other value than 0..3 is
 *               RVDD_ERR_ARG.  Per handle.
 *   "stream_reset_each": 1 = every step of rvdd_video_push carries the reset mark of every ready slot: non-recurrent checkpoints
 *               (--patch_depth 2, the model's training_unrollings == 1: recurrentModel.forward resets before every step,
 *               models/recurrent_model.py:233-245).  Default 0.  Acts on rvdd_video_push only.  Per handle.
 *   "stream_flow_from_denoised": 1 = --val_flow_from_denoised (validate.py:16-38, 81-82) in rvdd_video_push: after its frame-step a push
 *               takes rvdd_gray_of_rgb of the out_rgb it has just written (the handle's "bayer_pattern", the push's bit_depth) into a
 *               plane per slot, and the NEXT push forms the pair towards the previous frame of every ready slot whose previous push
 *               gave an output of the same video as (I0 = gray[centre], I1 = that plane) instead of (gray[centre], gray[previous]).
 *               A slot's first ready push keeps the noisy pair (the reference's first frame keeps the dataset's flow), and so does
 *               the pair towards the next frame: no output exists for that frame yet.  With "stream_reset_each" it applies all the
 *               same (the reference skips the online flow on FirstOfVideo only); with "no_warp" it changes nothing.  The plane is
 *               taken from out_rgb inside the push that wrote it, so the caller may overwrite out_rgb between pushes.  Still one
 *               asynchronous rvdd_tvl1flow_batch per push.  Default 0: exactly the launches of a push without it.  Acts on
 *               rvdd_video_push only.  Per handle.
 *   "stream_all_frames": 1 = rvdd_video_push outputs EVERY frame of a video, not only frames 1 .. N-1-future: the first frame on the
 *               push that completes 1 + future frames (previous frame = itself, zero flow towards it, reset mark), and with a future
 *               frame the last one on an IDLE pushed straight after it (next frame = itself, zero flow towards it); the contract is
 *               with rvdd_video_push.  Every other output keeps its bits.  Default 0: exactly the launches of a push without it, and
 *               nothing more allocated.  Acts on rvdd_video_push only.  Per handle.
 *   "stream_container": 1 / 2 = the `frames` of rvdd_video_push are packed bits in RVDD_BITS_MIPI / RVDD_BITS_MSB (the value is the
 *               enum rvdd_bits_order plus one): slot b's frame is the H * row_bytes bytes at byte b * H * row_bytes, read by
 *               rvdd_ingest_bits' kernel instead of rvdd_ingest_raw's; an IDLE slot's slice is not read.  The push must then say
 *               dtype RVDD_RAW_U16 (the samples' type), layout RVDD_RAW_MOSAIC and bit_depth 10 / 12 / 14, and MIPI at 10 / 14 bits
 *               needs an even W / 2: RVDD_ERR_ARG otherwise, and nothing is changed.  out_rgb and valid are bit for bit those of
 *               the same pushes with the unpacked uint16 frames, under every other stream option.  Default 0: exactly the
 *               launches of a push without it.  Any other value than 0..2 is RVDD_ERR_ARG.  Acts on rvdd_video_push only.  Per handle.
 * Every option belongs to the handle it is set on: no option changes what another handle of the process does.
 * Unknown names are an error. */
int rvdd_set_option(rvdd_t* h, const char* name, int32_t value);

/* Host-only helper of the TIFF reader that replaces `iio.read` (library.py:75-77): LZW strip / tile decoder
 * (TIFF 6.0 section 13).  in[n] -> out (capacity cap); returns the bytes produced or -1 (corrupt stream, output full). */
int64_t rvdd_tiff_lzw_decode(const uint8_t* in, int64_t n, uint8_t* out, int64_t cap);

/* ---- measurement ----------------------------------------------------------- */

/* When enabled, every launch of the U-Net kernels is bracketed by HIP events
 * on the launch stream.  rvdd_profile_read synchronises, accumulates and
 * returns, for kernel class `idx` (0..rvdd_profile_count()-1): its name, the
 * number of launches, the summed duration (ms) and the summed algorithmic
 * FLOPs and bytes since the last rvdd_profile_enable(h, 1). */
int rvdd_profile_enable(rvdd_t* h, int32_t on);
/* Restrict the bracketing to one kernel class (NULL = all) and to every
 * `stride`-th launch of a class: an event pair costs a few microseconds of
 * queue bubble, so a headline run samples the dominant kernel only. */
int rvdd_profile_select(rvdd_t* h, const char* kernel_class, int32_t stride);
int rvdd_profile_count(const rvdd_t* h);
int rvdd_profile_read(rvdd_t* h, int32_t idx, char* name, int32_t name_cap, int64_t* launches,
                      double* total_ms, double* flops, double* bytes);

/* HIP-event stopwatch on `stream` (bench.py times the whole step loop with it). */
int rvdd_timer_start(rvdd_t* h, void* stream);
int rvdd_timer_stop_ms(rvdd_t* h, void* stream, float* ms);   /* synchronises */

/* Kernel A/B hook: time `iters` back-to-back launches of the 48->48 3x3 conv +
 * ReLU (the dominant kernel) on the handle's own level-`level` maps with code
 * variant `variant` (0..2: code variants of the direct f32-MFMA kernel, 3: the Winograd f32-MFMA kernel, 4: the
 * split-f16 kernel, the default of the convunet); *ms = mean milliseconds per launch.  Synchronises. */
int rvdd_debug_conv_bench(rvdd_t* h, int32_t variant, int32_t level, int32_t iters, float* ms, void* stream);

const char* rvdd_version(void);

#ifdef __cplusplus
}
#endif
#endif /* RVDD_H */
