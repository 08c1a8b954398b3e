/* bsx.h — C ABI of libbsx.so, the MI355X-native backscrub hot path.
 *
 * Plain C: opaque handle, raw pointers, sizes.  No C++ / OpenCV / torch types cross this
 * boundary.  `d_` pointers are HIP device pointers on the context's GPU; `h_` pointers are
 * host memory.  `stream` is a hipStream_t passed as void* (NULL = the HIP default stream, as in every HIP API).
 * All functions return 0 on success or a negative BSX_E* code; nothing throws.
 *
 * What each entry point replaces in the reference (/root/reference):
 *
 *   bsx_version            bs_tensorflow_version()        lib/libbackscrub.h:13,  .cc:150-152
 *   bsx_new                bs_maskgen_new()               lib/libbackscrub.h:16-33, .cc:161-259
 *   bsx_delete             bs_maskgen_delete()            lib/libbackscrub.h:36,  .cc:261-277
 *   bsx_process_host       bs_maskgen_process()           lib/libbackscrub.h:39,  .cc:279-376
 *                          (one stream, host frame in, host mask out — what the C++ shim
 *                          csrc/bs_maskgen_shim.cpp forwards cv::Mat data to)
 *   bsx_process_batch      the same function for n_streams device-resident frames at once
 *   bsx_composite_batch    alpha_blend()                  app/deepseg.cc:108-134 (file-static)
 *   bsx_step_batch         one main-loop iteration        app/deepseg.cc:634-661
 *   bsx_step_batch_yuyv    … with convert_rgb_to_yuyv fused app/deepseg.cc:634-681
 *   bsx_step_batch_ex      … with cv::flip (and YUYV) fused  app/deepseg.cc:667-681; BSX_STEP_YUYV_IN: … and VideoCapture's YUYV->BGR  app/deepseg.cc:553,725
 *   bsx_step_batch_pipelined  … with the CalcMask worker's overlap of segmentation and blending  app/deepseg.cc:159-285, 634-661
 *   bsx_step_batch_vcam    … with the resize to the virtual camera's geometry (--vg) fused  app/deepseg.cc:634-681 (the resize: :675-679)
 *   bsx_step_batch_streams … for the streams that HAVE a new frame, addressed by id  app/deepseg.cc:182-216 (one filter step per new frame)
 *   bsx_step_batch_mixed   … with each stream's own settings: -b / -p bgblur / -H / -V and the s / h / v keys  app/deepseg.cc:387-437, 596-673, 777-790
 *   bsx_step_batch_vcam_mixed  … both: each stream's own settings, written at the virtual camera's geometry  app/deepseg.cc:387-437, 634-681
 *   bsx_new_geoms          bs_maskgen_new() for cameras of several capture sizes in ONE context  lib/libbackscrub.cc:161-259 (the ROIs of :234-246 once per size)
 *   bsx_new_geoms_ex       … with creation flags: BSX_GEOMS_EDGE_ROI admits sizes whose ROI is off the 4-pixel grid (segm_lite at 1920x1080)  lib/libbackscrub.cc:234-246
 *   bsx_step_batch_geoms   … for streams of different capture sizes together: one prep launch, one network pass, one tile launch  app/deepseg.cc:634-673
 *   bsx_step_batch_vcam_geoms  … the same streams, every composite written at the virtual camera's one size  app/deepseg.cc:634-681
 *   bsx_step_batch_vcam_geoms_outs  … the same streams, several outputs per stream, each of its own size (speaker + thumbnails, simulcast layers)
 *   bsx_step_batch_vcam_geoms_outs_nv12  … every output an NV12 surface with row pitches, for a video encoder (bsx_bgr_to_nv12: the stand-alone conversion)
 *   bsx_step_batch_surfaces  … every frame an NV12 surface too, as a video decoder leaves it: NV12 in, NV12 out (bsx_nv12_to_bgr: the stand-alone conversion)
 *   bsx_reset_streams      bsx_reset for a chosen subset of the streams (a slot reused for a new camera)
 *                          (set_input_frame → mask → alpha_blend), batched
 *   bsx_resize_bgr         grab_background() cv::resize   app/background.cc:178-194
 *   bsx_resize_bgr_batch   … of n images of their own sizes in one launch
 *   bsx_resize_surfaces_batch  … of n decoder surfaces (NV12), each to its own size: a video background's grab  app/background.cc:181-190
 *   bsx_bgr_to_yuyv        convert_rgb_to_yuyv()          app/deepseg.cc:87-106
 *   bsx_yuyv_to_bgr        VideoCapture's YUYV->BGR       app/deepseg.cc:553,725 (cv::COLOR_YUV2BGR_YUYV)
 *   bsx_nv12_to_bgr        the same integers for a video decoder's NV12 surface (pitched Y and UV planes)
 *   bsx_flip_bgr           cv::flip of the output frame   app/deepseg.cc:667-673 (flipHorizontal / flipVertical)
 *   bsx_gaussian_blur_bgr  cv::GaussianBlur of the background app/deepseg.cc:415-431,652-658 (-p bgblur:<n>: blur the camera frame itself
 *                          (or the background image) and composite over it)
 *   bsx_gaussian_blur_bgr_batch  cv::GaussianBlur of every camera's own frame, once per main-loop iteration  app/deepseg.cc:652-658
 *   bsx_gaussian_blur_surfaces_batch  … of every decoder surface (NV12), the blur mode of bsx_step_batch_surfaces  app/deepseg.cc:415-431, 652-661
 *   bsx_background_*       load_background / grab_background + reader thread   app/background.cc:29-104,126-194
 *   bsx_background_grab_batch  grab_background() of every camera's own source, once per main-loop iteration   app/deepseg.cc:648-651
 *   bsx_live_*             class CalcMask (worker thread, double buffering)     app/deepseg.cc:159-286
 *   bsx_profile_batch      the per-stage timers           app/deepseg.cc:137-156,701-720 (timinginfo_t)
 *   bsx_get_info           the geometry of backscrub_ctx_t lib/libbackscrub.cc:28-54,234-246
 *
 * Threading: a context is NOT thread-safe (same as the reference: one context per caller
 * thread, lib/libbackscrub.cc has no locks).  Callbacks fire synchronously on the calling
 * thread in the order prep → infer → mask, once per process call (per batch for the batched
 * calls), see lib/libbackscrub.cc:303,311,363.
 */
#ifndef BSX_H_
#define BSX_H_

#include <stddef.h>
#include <stdint.h>

/* The library is built with -fvisibility=hidden: the entry points below are its ONLY exported symbols (tests/test_cabi.py checks `nm -D`), so
 * linking it into an application adds nothing but `bsx_*` to that application's symbol namespace. */
#ifndef BSX_API
#define BSX_API __attribute__((visibility("default")))
#endif

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bsx_ctx bsx_ctx;

typedef void (*bsx_debug_fn)(void* caller_ctx, const char* msg);
typedef void (*bsx_stage_fn)(void* caller_ctx);

enum {
  BSX_OK = 0,
  BSX_EINVAL = -1,   /* NULL context / bad argument (reference: `return false`, .cc:280) */
  BSX_EMODEL = -2,   /* model file unreadable / unsupported op / unknown model type (.cc:191-203) */
  BSX_EDEVICE = -3,  /* HIP error (message via ondebug or stderr) */
  BSX_ESIZE = -4     /* frame geometry does not match the one given to bsx_new */
};

/* model types, as sniffed from the file name by the reference (lib/libbackscrub.cc:116-130) */
enum { BSX_MODEL_UNKNOWN = 0, BSX_MODEL_DEEPLAB = 1, BSX_MODEL_MLKIT = 2, BSX_MODEL_MEET = 3, BSX_MODEL_BODYPIX = 4 };

typedef struct bsx_info {
  int model_type;
  int width, height;              /* frame geometry */
  int n_streams;                  /* batch capacity */
  int in_w, in_h, in_c;           /* model input tensor */
  int out_w, out_h, out_c;        /* model output tensor */
  int roi[4];                     /* roidim   x,y,w,h in the frame       (.cc:234-246) */
  int in_roi[4];                  /* in_roidim x,y,w,h in the model canvas */
  int n_ops, n_steps;             /* graph operators / fused GPU launches per batch */
  int device;
  float norm_scale, norm_offset;  /* .cc:132-148 */
  double nn_flops_per_frame;      /* 2*MAC of the loaded graph */
  size_t act_bytes_per_stream;    /* activation arena per stream */
} bsx_info;

/* "bsx <ver> (HIP gfx950)"; static storage. */
BSX_API const char* bsx_version(void);

/* Number of visible HIP devices (0 if none / runtime missing). */
BSX_API int bsx_device_count(void);

/* Create a mask generator for `n_streams` independent camera streams of width x height BGR
 * frames on HIP device `device`.  `threads` is accepted for signature parity with
 * bs_maskgen_new (intra-op CPU threads there) and recorded only.  Callbacks may be NULL.
 * 1 <= n_streams <= 65535 (the stream index rides in a grid dimension).
 * Returns NULL on failure after reporting through ondebug (or stderr), like the reference. */
BSX_API bsx_ctx* bsx_new(const char* model_path, size_t threads, size_t width, size_t height,
                 int n_streams, int device,
                 bsx_debug_fn ondebug, bsx_stage_fn onprep, bsx_stage_fn oninfer, bsx_stage_fn onmask,
                 void* caller_ctx);

/* NULL-safe. */
BSX_API void bsx_delete(bsx_ctx* ctx);

BSX_API int bsx_get_info(const bsx_ctx* ctx, bsx_info* out);

/* Last error text for this context (or the global one if ctx==NULL); static/ctx storage. */
BSX_API const char* bsx_last_error(const bsx_ctx* ctx);

/* Reset the per-stream temporal state (`ofinal` → 0, `mask` → 255) of all streams.  bsx_reset_streams (below) resets a chosen subset. */
BSX_API int bsx_reset(bsx_ctx* ctx, void* stream);

/* Drop-in single-frame path.  h_bgr: height rows of width*3 bytes, `bgr_stride` bytes apart
 * (CV_8UC3 cv::Mat data/step).  h_mask: height rows of width bytes, `mask_stride` apart;
 * receives the full-frame mask (255 = background).  Uses stream slot `stream_idx`.
 * Synchronous: returns after the mask is in h_mask. */
BSX_API int bsx_process_host(bsx_ctx* ctx, int stream_idx, const uint8_t* h_bgr, size_t bgr_stride,
                     uint8_t* h_mask, size_t mask_stride);

/* Batched device path: frames [n][height][width][3] u8 contiguous (n <= n_streams; frame i
 * belongs to stream i — the dense contract; bsx_step_batch_streams, bsx_step_batch_mixed and bsx_step_batch_vcam_mixed take stream ids).  Updates each stream's temporal state and its persistent full-frame
 * mask.  If d_masks != NULL the masks are also copied there ([n][height][width]).
 * Asynchronous on `stream` unless callbacks are set (each callback needs a stream sync). */
BSX_API int bsx_process_batch(bsx_ctx* ctx, const uint8_t* d_frames, int n, uint8_t* d_masks, void* stream);

/* Device pointer of the persistent masks [n_streams][height][width] (a context of several classes: class after class, bsx_get_geom_info; valid until bsx_delete;
 * contents valid after the process call that produced them has completed on its stream) —
 * the analogue of `mask = ctx.mask` aliasing the lib-owned buffer (lib/libbackscrub.cc:374). */
BSX_API uint8_t* bsx_masks_device(bsx_ctx* ctx);

/* out = (bg*m + frame*(255-m))/255 per byte (C truncating divide).  d_bg is one
 * [height][width][3] image shared by all frames when bg_frame_stride == 0, else frame i uses
 * d_bg + i*bg_frame_stride.  d_masks == NULL means "use the context's persistent masks". */
BSX_API int bsx_composite_batch(bsx_ctx* ctx, const uint8_t* d_bg, size_t bg_frame_stride,
                        const uint8_t* d_frames, const uint8_t* d_masks, uint8_t* d_out, int n, void* stream);

/* bsx_process_batch followed by bsx_composite_batch on the same stream. */
BSX_API int bsx_step_batch(bsx_ctx* ctx, const uint8_t* d_frames, const uint8_t* d_bg, size_t bg_frame_stride,
                   uint8_t* d_out, int n, void* stream);

/* The same main-loop iteration with the composite leaving as YUYV 4:2:2 [n][height][width][2] (bytes Y0 V Y1 U): convert_rgb_to_yuyv
 * (app/deepseg.cc:87-106, applied at :681 right after alpha_blend) runs in the blend's epilogue — 2 B/px written instead of 3, and no separate
 * pass over the composite — for callers that feed a V4L2 YUYV sink.  Bit-identical to bsx_step_batch followed by bsx_bgr_to_yuyv.  width even. */
BSX_API int bsx_step_batch_yuyv(bsx_ctx* ctx, const uint8_t* d_frames, const uint8_t* d_bg, size_t bg_frame_stride,
                        uint8_t* d_out_yuyv, int n, void* stream);

/* The same iteration with the post steps of the main loop that sit between alpha_blend and the device write folded into WHERE the blend stores
 * its result (app/deepseg.cc:667-681): flags = BSX_STEP_FLIP_H | BSX_STEP_FLIP_V (cv::flip(raw, raw, 1 / 0 / -1) of the composite: the four pixels
 * a lane composites go to the mirrored column group in reverse order, the row to the mirrored row — no extra pass over the frame) and / or
 * BSX_STEP_YUYV (convert_rgb_to_yuyv of the — flipped — composite, as bsx_step_batch_yuyv).  flags = 0 is bsx_step_batch.  The persistent masks
 * are those of the unflipped camera frame, as in the reference.  Bit-identical to bsx_step_batch + bsx_flip_bgr [+ bsx_bgr_to_yuyv]. */
/* Aliasing: d_out == d_frames (the reference flips and composites `raw` in place, app/deepseg.cc:661-673) is allowed for every flag combination — with a flip or
 * YUYV flag and overlapping buffers the library composites into its own scratch first (the fused kernel would store to addresses another tile has not read
 * yet), so in-place costs one extra pass there; a plain composite runs in place at full speed.  Buffers that overlap PARTIALLY return BSX_EINVAL, and so does
 * BSX_STEP_BGBLUR with d_out == d_frames (every output pixel needs a neighbourhood of input pixels). */
#define BSX_STEP_YUYV 1u
#define BSX_STEP_FLIP_H 2u
#define BSX_STEP_FLIP_V 4u
/* BSX_STEP_NO_MASK: composite only — the full-resolution mask of this frame is formed in registers, blended and NOT stored (1 of the step's 7 HBM bytes per pixel).
 * Nothing later depends on it: every frame's mask is rebuilt from the model-resolution temporal state, which advances as usual; bsx_masks_device() then keeps
 * the last mask a call WITHOUT this flag stored.  For main loops that only need the composite (app/deepseg.cc:661 uses the mask for nothing else unless -d -d). */
#define BSX_STEP_NO_MASK 8u
/* BSX_STEP_YUYV_IN: d_frames holds the camera's RAW YUYV 4:2:2 frames, [n][height][width][2] bytes Y0 U Y1 V — what a V4L2 webcam delivers and what the reference's
 * capture converts with cv::COLOR_YUV2BGR_YUYV (CAP_PROP_CONVERT_RGB, app/deepseg.cc:553; explicit form :725) — instead of packed BGR.  The conversion (the integers
 * of bsx_yuyv_to_bgr) is folded into the two kernels that read the frame: the prep kernel converts the two taps of every resize sample, the mask tile kernel the four
 * pixels it composites, so the 3 B/px BGR frame is never written or read.  With BSX_STEP_YUYV the step is YUYV in -> YUYV out: 7 B/px of device traffic instead of 9
 * (frame 2 + background 3 in, composite 2 out) and 4 B/px over PCIe instead of 6.  Results are bit-identical to bsx_yuyv_to_bgr followed by the same step on the BGR
 * frames; that two-pass sequence is what runs, through a context-owned scratch, where the fused kernels do not apply (BSX_STEP_BGBLUR, a ROI that starts on an odd
 * column, width % 4 != 0, overlapping or unaligned buffers, an onmask callback).  width must be even.  Also accepted by bsx_step_batch_pipelined. */
#define BSX_STEP_YUYV_IN 16u
/* BSX_STEP_BGBLUR(ksize): the background of every stream is cv::GaussianBlur(its own camera frame, Size(ksize, ksize), 0) — `-p bgblur:<ksize>` without `-b`,
 * the reference's default way to run (app/deepseg.cc:652-661).  d_bg is ignored (may be NULL).  The blur and the alpha blend are ONE pass over the frames: each
 * tile of the blurred frame is composited while it is still in LDS, so the blurred image is never written or read back and the frame is read once, not twice.
 * Bit-identical to bsx_gaussian_blur_bgr into a per-stream background + bsx_step_batch_ex(flags) with bg_frame_stride = one frame; that two-call sequence is what
 * runs, on a context-owned scratch background, when the single pass does not apply (YUYV / flip flags, width % 4 != 0, unaligned buffers, ksize 1).  ksize odd, 1..31. */
#define BSX_STEP_BGBLUR(ksize) (((unsigned)(ksize) & 255u) << 8)
BSX_API int bsx_step_batch_ex(bsx_ctx* ctx, const uint8_t* d_frames, const uint8_t* d_bg, size_t bg_frame_stride,
                      uint8_t* d_out, int n, void* stream, unsigned flags);

/* One main-loop iteration for the streams named in ids[0..n): frame i, background i (bg_frame_stride as in bsx_step_batch_ex) and output i belong to stream
 * ids[i]; its temporal state and persistent mask are read and advanced in place; every other stream's state is untouched.  Every other batched entry point ties
 * batch position to state slot (frame i = stream i); a server whose cameras deliver at different rates, or join and leave, steps only the streams with a NEW frame
 * — the reference filters each frame once (CalcMask::run waits for a new frame, app/deepseg.cc:182-216; lib/libbackscrub.cc:315-356 advances once per call).
 *   - ids: host array of n distinct values in [0, n_streams), any order; read before the call returns (the caller may reuse it at once).  The library stages it
 *     through a small context-owned ring (pinned host + device memory, allocated on the first call): the host waits only when it runs several calls ahead of the GPU;
 *   - n == 0: returns 0 and enqueues nothing.  flags: exactly those of bsx_step_batch_ex (YUYV, FLIP_H / _V, NO_MASK, YUYV_IN, BGBLUR(k)), every route included;
 *   - result: bit-identical, per stream, to what that stream's frames would produce stepped alone (a one-stream context fed only its own frames); ids = 0 .. n-1
 *     is bsx_step_batch_ex(flags);
 *   - BSX_EINVAL, with a bsx_last_error text naming the offending position and value, for a duplicate id, an id out of range, n < 0 or n > n_streams; also for
 *     a pending pipelined composite and every argument bsx_step_batch_ex refuses.  All checks run on the host before anything is enqueued: a refused call changes
 *     no state.
 * bsx_step_batch_mixed and bsx_step_batch_vcam_mixed take the same ids (or NULL for the dense form); bsx_step_batch_pipelined, bsx_step_batch_vcam and
 * bsx_process_batch keep the dense contract (frame i = stream i). */
BSX_API int bsx_step_batch_streams(bsx_ctx* ctx, const int* ids, const uint8_t* d_frames, const uint8_t* d_bg, size_t bg_frame_stride,
                                   uint8_t* d_out, int n, void* stream, unsigned flags);

/* BSX_STREAM_FILTER_OFF: the reference with its filter switched off ('s' key, app/deepseg.cc:639-664, 782-783): the composite IS the camera frame (then
 * flipped / packed as set); the mask pipeline still runs, so the stream's temporal state and persistent mask advance exactly as with the filter on. */
#define BSX_STREAM_FILTER_OFF 32u
/* BSX_STREAM_YUYV_IN: THIS item's frame is the camera's raw YUYV 4:2:2 ([height_g][width_g][2] bytes Y0 U Y1 V) — BSX_STEP_YUYV_IN as a property of one position.
 * Taken only in items[i].setting.flags of bsx_step_batch_geoms and bsx_step_batch_vcam_geoms, whose positions each bring their own frame pointer; the mixed steps,
 * whose frames are one packed array with one layout, keep the batch flag and refuse this bit. */
#define BSX_STREAM_YUYV_IN 64u
typedef struct bsx_stream_setting {
  const uint8_t* d_bg;  /* [height][width][3] BGR on the context's device, 4-byte aligned; any number of streams may point at the same image */
  unsigned flags;       /* BSX_STEP_FLIP_H | BSX_STEP_FLIP_V | BSX_STEP_BGBLUR(k) | BSX_STREAM_FILTER_OFF */
} bsx_stream_setting;
/* One main-loop iteration of a batch whose streams do NOT share one setting — what one reference process per camera does with its own -b, -p bgblur, -H / -V
 * and its run-time s / h / v keys (app/deepseg.cc:387-437, 596-673, 777-790) — in ONE mask pipeline launch sequence and one tile launch:
 *   - ids: NULL = the dense contract (frame i is stream i); otherwise exactly the rules, staging and refusals of bsx_step_batch_streams;
 *   - flags (batch-wide, the buffer layouts): BSX_STEP_YUYV | BSX_STEP_NO_MASK | BSX_STEP_YUYV_IN only;
 *   - settings[0..n): host memory, read before the call returns; entry i belongs to position i.  The composite of position i (stream s):
 *     BSX_STREAM_FILTER_OFF: frame i itself; BSX_STEP_BGBLUR(k): alpha_blend(GaussianBlur(frame i, k), frame i, mask s) (d_bg is not read); otherwise
 *     alpha_blend(d_bg, frame i, mask s) — then the stream's own flip, then the YUYV pack if the batch asks for it.  A filter-off stream ignores its d_bg and blur
 *     size (toggling the filter is one bit, as the 's' key is), but a blur size that is set must still be valid;
 *   - result: per stream, composite, persistent mask and ofinal are bit-identical to bsx_step_batch_streams of that one stream with its d_bg and flags | its own
 *     flags; a filter-off stream's state and mask are those of that call with any background, its composite the frame (converted from YUYV with
 *     BSX_STEP_YUYV_IN) flipped as bsx_flip_bgr and packed as bsx_bgr_to_yuyv;
 *   - n == 0: returns 0 and enqueues nothing;
 *   - BSX_EINVAL before anything is enqueued, with a bsx_last_error text naming the position and value, for: the ids errors of bsx_step_batch_streams; settings
 *     NULL with n > 0; a flag bit outside the sets above (a stream's or the batch's); a blur size that is even or above 31; a NULL or unaligned d_bg on a stream that
 *     reads it; d_out overlapping d_frames or any stream's background (there is no in-place form); a pending pipelined composite; an odd width with YUYV out or in;
 *     and every context or buffer the fused tile route does not take (width, roi.x, roi.w multiples of 4, 4-byte aligned buffers, no onmask callback). */
BSX_API int bsx_step_batch_mixed(bsx_ctx* ctx, const int* ids, const uint8_t* d_frames, const bsx_stream_setting* settings,
                                 uint8_t* d_out, int n, void* stream, unsigned flags);

/* ---- cameras of different capture sizes in one context ----
 * Nothing in the network depends on the capture size: only the two ends of the pipeline see the frame (the ROI down-scale into the model canvas, and the mask
 * up-scale + blur + blend).  A context made by bsx_new_geoms holds up to BSX_MAX_GEOMS geometry classes (capture sizes); weights, arena, network buffers, compiled
 * kernels and the model-resolution temporal state exist once, every class has its own ROIs, resize tables and its own slice of the persistent masks.
 *   - streams are numbered class after class: class g owns ids [first_g, first_g + geoms[g].n_streams), first_0 = 0;
 *   - n_geoms == 1 IS bsx_new(model_path, threads, width, height, n_streams, ...): the same context, every entry point as before;
 *   - returns NULL, with a message (through ondebug or stderr, and bsx_last_error(NULL)) that names the class index and its size, for: n_geoms outside
 *     [1, BSX_MAX_GEOMS]; a non-positive size or stream count; two classes of the same size; more than 65535 streams in total; an onmask callback with more than one
 *     class; and, with more than one class, a class the fused tile route does not take (width, roi.x and roi.w multiples of 4 and a tiled linear mask up-scale: the rule
 *     bsx_step_batch_mixed applies per call, applied at creation).  With segm_lite (160 x 96, its ratio held as a float) the reference's ROI arithmetic gives some
 *     16:9 sizes a ROI width that is no multiple of 4 — 1920x1080 -> 1799, 960x540 -> 899, 848x480 -> 799 — and those are refused; 1280x720 and 640x360 are fine
 *     (bsx_new_geoms_ex with BSX_GEOMS_EDGE_ROI, below, takes them);
 *   - on a context of more than one class these work: bsx_step_batch_geoms, bsx_step_batch_vcam_geoms, bsx_reset, bsx_reset_streams, bsx_get_info (class 0's
 *     geometry, the total n_streams), bsx_geom_count / bsx_get_geom_info, bsx_masks_device, bsx_last_error, bsx_delete, bsx_plan_describe, bsx_debug_buffer (0-2 as always; 3 = the whole mask
 *     allocation), bsx_debug_tensor*, and everything that takes its own w, h (bsx_resize_bgr*, bsx_bgr_to_yuyv, bsx_yuyv_to_bgr, bsx_flip_bgr, bsx_gaussian_blur_bgr,
 *     bsx_gaussian_blur_bgr_batch,
 *     bsx_background_*).  Every other entry point — the dense, by-id, mixed, vcam and pipelined steps, process, composite, profile, live, the debug stages and tile
 *     statistics — returns BSX_EINVAL ("context has N geometries"; bsx_live_new: NULL) and enqueues nothing. */
#define BSX_MAX_GEOMS 8
typedef struct bsx_geometry { int width, height, n_streams; } bsx_geometry;
BSX_API bsx_ctx* bsx_new_geoms(const char* model_path, size_t threads, const bsx_geometry* geoms, int n_geoms, int device,
                               bsx_debug_fn ondebug, bsx_stage_fn onprep, bsx_stage_fn oninfer, bsx_stage_fn onmask, void* caller_ctx);

/* bsx_new_geoms with creation flags.  flags == 0 IS bsx_new_geoms; a bit that is not listed here returns NULL with a message that names the bit.
 *   BSX_GEOMS_EDGE_ROI  take classes whose ROI is off the 4-pixel grid: for any n_geoms from 1 up a class is admitted when its width is a multiple of 4 and its mask
 *     up-scale is the tiled linear one; roi.x and roi.w are free (segm_lite at 1920x1080, 960x540, 848x480 and 1600x900, MLKit at 960x540 and 1600x900).  Still
 *     refused, with the class index, its size and the value: a width that is no multiple of 4 (a row would not be whole dwords), and a class without the tiled
 *     up-scale.  On such a context bsx_step_batch_geoms and bsx_step_batch_vcam_geoms take streams of those classes under all their other rules (4-byte aligned
 *     d_frame / d_out / d_bg, no overlap, no blur bit, no onmask; a BSX_STREAM_YUYV_IN item still needs an even roi.x and a proper INTER_LINEAR down-scale, so
 *     1920x1080 lite passes and a class with an odd roi.x is refused per item), with what they always compute: per stream byte-identical to
 *     bsx_step_batch_streams of that stream in a one-geometry context of its size.  The launch count is unchanged; a call that touches such a class runs kernels
 *     that anchor the composite's 4-pixel groups to the frame, a call that touches none runs exactly what it runs on a bsx_new_geoms context.  Every other entry
 *     point behaves as on any context of that class count (bsx_step_batch_mixed keeps refusing a ROI off the grid). */
#define BSX_GEOMS_EDGE_ROI 1u
BSX_API bsx_ctx* bsx_new_geoms_ex(const char* model_path, size_t threads, const bsx_geometry* geoms, int n_geoms, int device, unsigned flags,
                                  bsx_debug_fn ondebug, bsx_stage_fn onprep, bsx_stage_fn oninfer, bsx_stage_fn onmask, void* caller_ctx);

/* The classes of a context (1 for one made by bsx_new) and the geometry of class g.  The persistent mask of stream s of class g is
 * bsx_masks_device() + mask_offset + (s - first_stream) * width * height. */
typedef struct bsx_geom_info {
  int width, height, n_streams, first_stream;
  int roi[4], in_roi[4];          /* as bsx_info, for this class */
  size_t mask_offset;             /* bytes from bsx_masks_device() to the class's [n_streams][height][width] masks */
} bsx_geom_info;
BSX_API int bsx_geom_count(const bsx_ctx* ctx);
BSX_API int bsx_get_geom_info(const bsx_ctx* ctx, int g, bsx_geom_info* out);

/* One main-loop iteration for the streams named in ids[0..n), of ANY mix of the context's classes, each with its own buffers and settings — in one prep launch, one
 * pass of the network, one tile-class and one tile launch (and at most one launch for the strips outside the ROIs), whatever the number of classes.
 *   - ids: required (the id decides the class): n distinct ids in any order, classes may interleave; rules, staging ring and refusal texts of bsx_step_batch_streams;
 *   - items[0..n): host memory, read before the call returns; entry i belongs to stream ids[i].  d_frame / d_out / setting.d_bg have the capture size of THAT stream's
 *     class; setting.flags: BSX_STEP_FLIP_H | BSX_STEP_FLIP_V | BSX_STREAM_FILTER_OFF | BSX_STREAM_YUYV_IN;
 *   - the pixel format belongs to the item: with BSX_STREAM_YUYV_IN items[i].d_frame is that camera's raw YUYV 4:2:2, [height_g][width_g][2] bytes Y0 U Y1 V, and
 *     cv::COLOR_YUV2BGR_YUYV (app/deepseg.cc:553, :725) is folded into the kernels that read it — no BGR frame exists; without the bit the frame is BGR.  Any mix of
 *     the two formats in one call, with every other setting bit and batch flag.  A call with no YUYV item launches exactly the kernels it launched before the bit
 *     existed; one YUYV item switches the call's prep, tile and outside-ROI launches to forms that read the format per position (still one launch each).  A
 *     filter-off YUYV item's composite is its frame converted, then flipped and packed as set, inside the ROI and on the strips outside it;
 *   - flags (batch-wide, the output layout and the mask store): BSX_STEP_YUYV | BSX_STEP_NO_MASK;
 *   - result, per stream: composite, persistent mask and ofinal are bit-identical to bsx_step_batch_mixed of that one stream in a one-geometry context of its size
 *     with the same setting and flags (BSX_STEP_YUYV_IN there for a YUYV item) — and so to this call with that item's frame first converted by bsx_yuyv_to_bgr.
 *     Other streams' state is untouched;
 *   - works on every context, also one made by bsx_new (then it is the mixed step with per-position pointers instead of packed arrays);
 *   - n == 0: returns 0 and enqueues nothing;
 *   - BSX_EINVAL before anything is enqueued, with a bsx_last_error text naming the position and value, for: the ids errors of bsx_step_batch_streams; items NULL; a
 *     NULL or not 4-byte aligned d_frame, d_out, or d_bg that is read; a flag bit outside the sets above (BSX_STEP_BGBLUR in a setting is not taken, and neither is
 *     the batch flag BSX_STEP_YUYV_IN: the format is the item's); an odd class width with YUYV out; an output overlapping any frame (over its real extent: W*H*2
 *     bytes for a YUYV item), background or other output of the call; a pending pipelined composite; an onmask callback; a stream whose class is off the fused tile
 *     route (possible only in a one-class context); a YUYV item whose class has no fused YUYV prep — a down-scale table that is not INTER_LINEAR proper (capture
 *     ROI equal to the model ROI: a copy; exactly twice it: the 2x2 area mean), an odd width or ROI column.  The text names items[i], the stream, the class size and
 *     the table; the caller converts that stream with bsx_yuyv_to_bgr and passes BGR (the library has no conversion fallback here).  A refused call changes no state. */
typedef struct bsx_geom_item {
  const uint8_t* d_frame;       /* [height_g][width_g][3] BGR of the stream's class, or [height_g][width_g][2] YUYV with BSX_STREAM_YUYV_IN; 4-byte aligned */
  uint8_t* d_out;               /* [height_g][width_g][3], or [..][2] with BSX_STEP_YUYV, 4-byte aligned */
  bsx_stream_setting setting;   /* d_bg at the capture size of that class; BSX_STEP_FLIP_H | BSX_STEP_FLIP_V | BSX_STREAM_FILTER_OFF | BSX_STREAM_YUYV_IN */
} bsx_geom_item;
BSX_API int bsx_step_batch_geoms(bsx_ctx* ctx, const int* ids, const bsx_geom_item* items, int n, void* stream, unsigned flags);

/* bsx_step_batch_geoms with every composite written at ONE common size, the virtual camera's (--vg, app/deepseg.cc:674-681): a conference or gallery server that
 * takes cameras of several capture sizes and sends every participant out at out_w x out_h.  One prep launch, one pass of the network, one tile-class launch, one
 * masks-only tile launch and ONE resize pass that reads each position's frame, background and mask taps and writes its output, whatever the number of classes:
 * no capture-size composite, no full-size resized image, no caller-owned scratch, no host synchronisation.
 *   - ids, items: the rules of bsx_step_batch_geoms (required ids, any order, classes may interleave, the same staging ring).  items[i].d_frame and
 *     items[i].setting.d_bg have the capture size of the class of ids[i]; items[i].d_out is [out_h][out_w][3], or [out_h][out_w][2] with BSX_STEP_YUYV — the same
 *     size for every position; setting.flags: BSX_STEP_FLIP_H | BSX_STEP_FLIP_V | BSX_STREAM_FILTER_OFF | BSX_STREAM_YUYV_IN (that item's d_frame is YUYV 4:2:2,
 *     [height_g][width_g][2]: the rules of bsx_step_batch_geoms; the resize pass converts the taps it reads, the masks-only tile launch reads no frame);
 *   - flags (batch-wide): BSX_STEP_YUYV only;
 *   - result, per stream: the output is byte-identical to bsx_resize_bgr(C, W_g, H_g -> out_w, out_h) [then bsx_bgr_to_yuyv], C being the BGR composite
 *     bsx_step_batch_geoms writes for the same item, its flip included — blend -> flip -> resize -> pack, the order of bsx_step_batch_vcam (an exact 2x down-scale is
 *     the 2x2 area mean; an output of a class's own size is that class's composite).  The persistent mask and ofinal of every stream of the context, those that
 *     sit out included, are byte-identical to that call's;
 *   - the per-class capture -> output tables of each (out_w, out_h) are built and uploaded on the first call at that size and kept by the context;
 *   - works on every context, also one made by bsx_new (then it is bsx_step_batch_vcam_mixed with per-position pointers);
 *   - n == 0: returns 0 and enqueues nothing;
 *   - BSX_EINVAL before anything is enqueued, with a bsx_last_error text naming the position and value, for: the ids errors of bsx_step_batch_streams; items NULL;
 *     out_w or out_h <= 0; BSX_STEP_NO_MASK (it has no vcam form), BSX_STEP_YUYV_IN (the format is the item's) and any other batch flag bit; a blur size or a
 *     foreign bit in a setting; a NULL or not 4-byte aligned d_frame, d_out, or d_bg that is read; an odd out_w with BSX_STEP_YUYV; an output (out_w x out_h)
 *     overlapping any frame (W*H*2 bytes for a YUYV item), background or other output of the call; a pending pipelined composite; an onmask callback; a stream whose
 *     class is off the fused tile route (possible only in a one-class context, which bsx_step_batch_vcam_mixed takes); a YUYV item whose class has no fused YUYV
 *     prep (as bsx_step_batch_geoms).  A refused call changes no state.  BSX_EDEVICE for a batch of 2^31 workgroups or more. */
BSX_API int bsx_step_batch_vcam_geoms(bsx_ctx* ctx, const int* ids, const bsx_geom_item* items, int n, int out_w, int out_h, void* stream, unsigned flags);

/* bsx_step_batch_vcam_geoms with SEVERAL outputs per stream, each of its own size: a gallery that shows the active speaker at 1280x720 and everyone else at 320x180,
 * a simulcast forwarder that publishes every camera at 640x360, 320x180 and 160x90.  Each stream is filtered ONCE (one prep launch, one pass of the network, one
 * tile-class launch, one masks-only tile launch); ONE resize pass then writes every output record from its item's frame, background and mask taps — its grid ranges
 * over the records, each with the tiles of its own size.  No capture-size composite is stored and none is read back per layer.
 *   - ids, items[0..n): the rules of bsx_step_batch_vcam_geoms (required ids, any order, classes may interleave, the same staging ring; setting.flags:
 *     BSX_STEP_FLIP_H | BSX_STEP_FLIP_V | BSX_STREAM_FILTER_OFF | BSX_STREAM_YUYV_IN, no blur).  items[i].d_out is NOT read;
 *   - outs[0..m): host memory, read before the call returns, in any order.  outs[j] asks for the composite of items[outs[j].item] at out_w x out_h in d_out:
 *     [out_h][out_w][3], or [out_h][out_w][2] with BSX_STEP_YUYV, 4-byte aligned.  An item may be named by 0 to BSX_MAX_OUTS_PER_ITEM records (with none its stream
 *     still advances and its persistent mask is still written; two records may ask for the same size in different buffers); a call uses at most BSX_MAX_OUT_SIZES
 *     distinct sizes;
 *   - flags (batch-wide): BSX_STEP_YUYV only;
 *   - result: every outs[j].d_out is byte-identical to what bsx_step_batch_vcam_geoms(.., out_w, out_h, ..) writes for that item; persistent mask and ofinal of every
 *     stream of the context are byte-identical to bsx_step_batch_geoms'.  Each stream advances once, however many records name it;
 *   - the per-class tables of each size come from the cache bsx_step_batch_vcam_geoms fills: a size seen before allocates and uploads nothing.  Records and
 *     (class, size) groups travel through the staging ring: no host synchronisation unless the caller runs four calls ahead;
 *   - works on every context (bsx_new, bsx_new_geoms, bsx_new_geoms_ex with BSX_GEOMS_EDGE_ROI);
 *   - n == 0: returns 0 and enqueues nothing.  m == 0 with n > 0 is a masks-only step;
 *   - BSX_EINVAL before anything is enqueued, with a bsx_last_error text naming outs[j] or items[i] and the value, for: every refusal of bsx_step_batch_vcam_geoms
 *     that still applies (ids, items NULL, flag bits, a NULL or unaligned d_frame or d_bg that is read, a pending pipelined composite, an onmask callback, a class
 *     off the fused route, a YUYV item without a fused YUYV prep); outs NULL with m > 0; m < 0; an item outside [0, n); a fifth record for one item; a fifth
 *     distinct size; a non-positive size; an odd out_w with BSX_STEP_YUYV; a NULL or not 4-byte aligned d_out; an output overlapping any frame (W*H*2 bytes for a
 *     YUYV item), background or other output of the call.  A refused call changes no state.  BSX_EDEVICE for a batch of 2^31 workgroups or more. */
#define BSX_MAX_OUT_SIZES 4        /* distinct (out_w, out_h) in one call */
#define BSX_MAX_OUTS_PER_ITEM 4    /* output records that may name one item */
typedef struct bsx_vcam_out { int item; int out_w, out_h; uint8_t* d_out; } bsx_vcam_out;
BSX_API int bsx_step_batch_vcam_geoms_outs(bsx_ctx* ctx, const int* ids, const bsx_geom_item* items, int n, const bsx_vcam_out* outs, int m, void* stream,
                                           unsigned flags);

/* bsx_step_batch_vcam_geoms_outs writing every record as an NV12 SURFACE: a Y plane and an interleaved UV plane of half the rows, each with a row pitch — what a
 * video encoder takes (a 160-wide simulcast layer in rows of 256 bytes).  The resize pass holds each group of four output pixels as B, G, R when it packs them; it
 * stores Y and 2x2-subsampled chroma from there, 1.5 B/px, instead of a packed image that one conversion pass per layer size would read back.
 * The definition.  No reference code writes 4:2:0, so NV12 is derived from the reference's own 4:2:2 packer: an NV12 output is a pure function of the YUYV output the
 * library already produces.  For an output image C (BGR, out_w x out_h, both even) let Q = bsx_bgr_to_yuyv(C): [out_h][out_w / 2] words of bytes (Y0, Ca, Y1, Cb),
 * the bytes of convert_rgb_to_yuyv (app/deepseg.cc:87-106).  Then
 *     Y[y][2c] = Q[y][c].Y0,  Y[y][2c + 1] = Q[y][c].Y1                                            [out_h] rows of pitch_y bytes
 *     UV[r][2c] = (Q[2r][c].Ca + Q[2r + 1][c].Ca) / 2,  UV[r][2c + 1] = (Q[2r][c].Cb + Q[2r + 1][c].Cb) / 2      [out_h / 2] rows of pitch_uv bytes
 * the division integer and truncating: the reference's own averaging of two chroma samples (deepseg.cc:98-99) applied to the two rows.  Ca is the byte a YUYV
 * consumer reads as U, so the plane is U, V interleaved: NV12.  Bytes [out_w, pitch) of every row of both planes are NOT written.
 *   - everything of bsx_step_batch_vcam_geoms_outs but the output form: the ids / items rules, BSX_MAX_OUTS_PER_ITEM and BSX_MAX_OUT_SIZES, the table cache and the
 *     staging ring (no host synchronisation unless four calls ahead), the front (one prep launch, the network, one tile-class launch, one masks-only tile launch),
 *     ONE resize pass over all records;
 *   - result: the planes of outs[j] are the definition applied to the BGR image bsx_step_batch_vcam_geoms_outs writes for that item at that size; persistent masks
 *     and ofinal of every stream of the context are byte-identical to bsx_step_batch_geoms'.  Works on every context (bsx_new, bsx_new_geoms, bsx_new_geoms_ex with
 *     BSX_GEOMS_EDGE_ROI).  n == 0: returns 0 and enqueues nothing.  m == 0 with n > 0 is a masks-only step;
 *   - flags: 0;
 *   - BSX_EINVAL before anything is enqueued, with a bsx_last_error text naming outs[j] or items[i] and the value, for: every refusal of
 *     bsx_step_batch_vcam_geoms_outs that still applies; any bit in flags; an odd out_w or out_h; a pitch below out_w or not a multiple of 4; a NULL or not 4-byte
 *     aligned plane; a plane overlapping any frame, background or other plane of the call, its own record's second plane included.  A refused call changes no state;
 *   - overlap is judged on a plane's byte extent pitch * (rows - 1) + out_w: two records that interleave their rows inside one canvas are refused.
 * Out of scope: writing a mosaic (several records into one canvas), I420 / three-plane output, odd sizes.  (NV12 input: bsx_step_batch_surfaces.) */
typedef struct bsx_vcam_out_nv12 {
  int item; int out_w, out_h;          /* as bsx_vcam_out; out_w and out_h even */
  int pitch_y, pitch_uv;               /* bytes per row of each plane: multiples of 4, >= out_w */
  uint8_t* d_y;                        /* [out_h][pitch_y], 4-byte aligned */
  uint8_t* d_uv;                       /* [out_h / 2][pitch_uv], 4-byte aligned */
} bsx_vcam_out_nv12;
BSX_API int bsx_step_batch_vcam_geoms_outs_nv12(bsx_ctx* ctx, const int* ids, const bsx_geom_item* items, int n, const bsx_vcam_out_nv12* outs, int m, void* stream,
                                                unsigned flags /* 0 */);

/* bsx_step_batch_vcam_geoms_outs_nv12 whose FRAMES are NV12 surfaces as well: what a simulcast forwarder holds after the hardware decoder — a Y plane and an
 * interleaved UV plane of half the rows, each with a row pitch — stepped straight into encoder surfaces.  The prep kernel and the resize pass read 1.5 B/px from the
 * decoder's surface; no 3 B/px BGR frame is stored or read back.
 * The definition.  No reference code reads 4:2:0, so an NV12 frame is defined through the 4:2:2 frame the library already takes.  For a capture of W x H, both even,
 * with planes Y ([H] rows of pitch_y bytes) and UV ([H / 2] rows of pitch_uv bytes) let Q be the YUYV image [H][W / 2] of words (Y0 U Y1 V) with
 *     Q[y][c] = ( Y[y][2c],  UV[y / 2][2c],  Y[y][2c + 1],  UV[y / 2][2c + 1] )
 * The BGR frame of the surface is bsx_yuyv_to_bgr(Q): every pixel takes the chroma pair of its 2 x 2 block, nothing is interpolated, and the integers are those of
 * cv::COLOR_YUV2BGR_YUYV.  (Believed, not checked: this is also what cv::COLOR_YUV2BGR_NV12 computes, since OpenCV uses the same BT.601 fixed-point constants for
 * both layouts.  Nothing here depends on it.)  Bytes [W, pitch) of a row mean nothing and are never read.  bsx_nv12_to_bgr is that conversion on its own.
 *   - everything of bsx_step_batch_vcam_geoms_outs_nv12 but the frame's form: the ids rules and the staging ring (no host synchronisation unless four calls ahead),
 *     BSX_MAX_OUTS_PER_ITEM, BSX_MAX_OUT_SIZES and the per-size table cache, every refusal of an output record, n == 0 (returns 0, enqueues nothing), m == 0 with
 *     n > 0 (a masks-only step), every kind of context (bsx_new, bsx_new_geoms, bsx_new_geoms_ex with BSX_GEOMS_EDGE_ROI).  Launches: ONE prep launch, the network, one
 *     tile-class launch, one masks-only tile launch, ONE resize pass;
 *   - result: every output plane, every persistent mask and ofinal of every stream of the context are byte-identical to bsx_step_batch_vcam_geoms_outs_nv12 fed the
 *     BGR frames bsx_nv12_to_bgr makes of the same surfaces.  A filter-off item's output is its converted frame, flipped, resized and packed;
 *   - admission of a class: the proper INTER_LINEAR down-scale table (the condition of a BSX_STREAM_YUYV_IN item: not the copy, not the 2x2 area mean), an even width
 *     and height, a width of at least 4.  Chroma is addressed by the FRAME's column and row, (roi.x + sx) >> 1 and (roi.y + sy) >> 1, so an odd roi.x or roi.y — the
 *     edge classes, segm_lite at 1920 x 1080 — needs no further rule.  There is no conversion fallback: an item of a class that is not admitted is refused with a text
 *     naming items[i], the stream, the class size and the reason, and the caller converts with bsx_nv12_to_bgr and takes bsx_step_batch_vcam_geoms_outs_nv12;
 *   - setting.flags: BSX_STEP_FLIP_H | BSX_STEP_FLIP_V | BSX_STREAM_FILTER_OFF; setting.d_bg: BGR at the class's capture size, 4-byte aligned, unread with
 *     BSX_STREAM_FILTER_OFF; flags: 0;
 *   - BSX_EINVAL before anything is enqueued, with a bsx_last_error text naming items[i] or outs[j] and the value, for: items NULL; a NULL or not 4-byte aligned
 *     plane; a pitch below the class's width or not a multiple of 4 (or a plane of 2 GiB or more); a setting bit outside the three above, BSX_STREAM_YUYV_IN and a
 *     blur size included; any bit in flags; a NULL or unaligned d_bg that is read; a pending pipelined composite, an onmask callback, a class off the fused route; an
 *     output plane overlapping an input plane, a background or another output plane.  An input plane is judged on its extent pitch * (rows - 1) + W.  A refused
 *     call changes no state.
 * Out of scope: NV12 items mixed with BGR or YUYV items in one call; NV12 input for the capture-size steps (bsx_step_batch_geoms) and for the packed-output vcam
 * calls; P010 and I420; odd sizes; a surface whose two planes share one pitch field. */
typedef struct bsx_surface_item {
  const uint8_t* d_y;                  /* [height_g] rows of pitch_y bytes, 4-byte aligned */
  const uint8_t* d_uv;                 /* [height_g / 2] rows of pitch_uv bytes (U, V interleaved), 4-byte aligned */
  int pitch_y, pitch_uv;               /* multiples of 4, >= width_g */
  bsx_stream_setting setting;          /* d_bg: BGR at the class's capture size; BSX_STEP_FLIP_H | BSX_STEP_FLIP_V | BSX_STREAM_FILTER_OFF */
} bsx_surface_item;
BSX_API int bsx_step_batch_surfaces(bsx_ctx* ctx, const int* ids, const bsx_surface_item* items, int n, const bsx_vcam_out_nv12* outs, int m, void* stream,
                                    unsigned flags /* 0 */);

/* Reset the temporal state of the listed streams only (ofinal → 0, persistent mask → 255, as bsx_reset does for all) — a slot reused for a new camera.  The
 * other streams' state is untouched, and a pending pipelined composite is NOT dropped: the call is refused (BSX_EINVAL) while one is pending.  Same ids rules,
 * errors and staging as bsx_step_batch_streams; asynchronous on `stream`. */
BSX_API int bsx_reset_streams(bsx_ctx* ctx, const int* ids, int n, void* stream);

/* Throughput mode — the same main-loop iteration as a TWO-DEEP PIPELINE (dense contract: frame i = stream i).  The reference runs its two halves concurrently: CalcMask::run() segments on a
 * worker thread (app/deepseg.cc:182-216) while the capture loop blends and writes (:634-681).  Call k enqueues the mask pipeline (prep → network → decode /
 * temporal filter) of batch k on `stream` and, concurrently on a context-owned low-priority stream, the mask up-scale + blur + composite of batch k - 1 — the
 * HBM-bound half fills the gaps of the latency-bound half instead of waiting behind it.  Every frame is still composited with ITS OWN mask (the reference's
 * loop blends with whatever mask is newest): outputs, persistent masks and temporal state are bit-identical to bsx_step_batch_ex(flags), one call later.
 *   - d_out(k) and bsx_masks_device() hold batch k's results once call k + 1 (or the flush) has completed on `stream`;
 *   - d_frames(k), d_bg(k) and d_out(k) must stay valid and unmodified until then; d_out must not overlap d_frames;
 *   - d_frames == NULL flushes: the pending composite runs on `stream` (all other arguments ignored); bsx_reset drops it;
 *   - `stream` may differ from call to call (double-buffered callers): every call records the end of its mask pipeline on its own stream, and the composite of
 *     that batch, the next call's network (it reuses the arena) and the flush wait for THAT event — the caller orders nothing across its streams;
 *   - flags: BSX_STEP_YUYV | BSX_STEP_FLIP_H | BSX_STEP_FLIP_V | BSX_STEP_NO_MASK | BSX_STEP_YUYV_IN (no BSX_STEP_BGBLUR); the geometry must be the fused tile kernel's
 *     (width, roi.x, roi.w multiples of 4, 4-byte aligned buffers) and no stage callback may be set — otherwise BSX_EINVAL, as does every other entry point
 *     that advances the temporal state while a composite is pending (bsx_process_batch / _host, bsx_step_batch*, bsx_profile_batch, bsx_debug_run_stage 1-3). */
BSX_API int bsx_step_batch_pipelined(bsx_ctx* ctx, const uint8_t* d_frames, const uint8_t* d_bg, size_t bg_frame_stride,
                             uint8_t* d_out, int n, void* stream, unsigned flags);

/* One main-loop iteration whose output has the VIRTUAL CAMERA's geometry (--vg differs from the capture size, app/deepseg.cc:675-679; dense contract: frame i = stream i).  For every stream, in the
 * reference's order: C = alpha_blend(bg, frame, mask) at the capture size; F = cv::flip(C) with BSX_STEP_FLIP_H / _V; R = cv::resize(F, Size(out_w, out_h))
 * with INTER_LINEAR (the 2x2 area mean when both scales are exactly 2 — the integers of bsx_resize_bgr); convert_rgb_to_yuyv(R) with BSX_STEP_YUYV.
 * d_out is [n][out_h][out_w][3], or [n][out_h][out_w][2] with BSX_STEP_YUYV.  The masks are made as bsx_process_batch makes them (persistent masks, temporal
 * state and stage callbacks exactly as bsx_step_batch_ex(flags)); then ONE pass reads frame, background and mask taps and writes the output: neither the
 * capture-size composite nor the full-size resized image is stored.  The flip is applied before the resize (resize(flip(C)) and flip(resize(C)) differ at
 * ratios such as 640 -> 426).  The table of each (out_w, out_h) is built on its first use and kept by the context.
 *   - flags: BSX_STEP_YUYV | BSX_STEP_FLIP_H | BSX_STEP_FLIP_V | BSX_STEP_YUYV_IN | BSX_STEP_BGBLUR(k); BSX_STEP_NO_MASK is refused;
 *   - BSX_EINVAL also for out_w or out_h <= 0, an odd out_w with BSX_STEP_YUYV, an odd capture width with BSX_STEP_YUYV_IN, d_out overlapping d_frames or
 *     d_bg (no in-place form: each output pixel reads a neighbourhood of input pixels), and a pending pipelined composite — all before any state changes;
 *   - out_w == width and out_h == height: the call IS bsx_step_batch_ex(flags). */
BSX_API int bsx_step_batch_vcam(bsx_ctx* ctx, const uint8_t* d_frames, const uint8_t* d_bg, size_t bg_frame_stride,
                                uint8_t* d_out, int out_w, int out_h, int n, void* stream, unsigned flags);

/* bsx_step_batch_vcam for a chosen subset of the streams, each with its OWN settings — one reference process per camera with its own -b, -p bgblur, -H / -V,
 * its s / h / v keys AND its --vg — in one mask pipeline and ONE pass that reads each position's descriptor, frame, background and mask taps and writes the
 * output at (out_w, out_h): no capture-size composite, no full-size resized image, no caller-owned scratch.
 *   - ids: NULL = the dense contract (frame i is stream i); otherwise exactly the rules, staging ring and refusals of bsx_step_batch_streams: the temporal state
 *     and persistent mask of stream ids[i] advance in place, every other stream is untouched;
 *   - settings[0..n): the bsx_stream_setting of bsx_step_batch_mixed, same flag set and meaning (d_bg: a capture-size background; BSX_STEP_FLIP_H | BSX_STEP_FLIP_V |
 *     BSX_STEP_BGBLUR(k) | BSX_STREAM_FILTER_OFF); here d_bg may lie at any address (an unaligned image costs its own stream the byte-wise loads);
 *   - flags (batch-wide, the buffer layouts): BSX_STEP_YUYV | BSX_STEP_YUYV_IN only; BSX_STEP_NO_MASK is refused, as bsx_step_batch_vcam refuses it;
 *   - d_out: [n][out_h][out_w][3], or [..][2] with BSX_STEP_YUYV — one output size per call;
 *   - result for position i (stream s), in the reference's order: C = the capture-size composite bsx_step_batch_mixed defines for settings[i] (the blend over
 *     d_bg, over the blur of the stream's own frame, or — filter off — the frame itself: neither background nor mask is read); F = cv::flip(C) with the stream's
 *     own flip bits; R = cv::resize(F, Size(out_w, out_h)) with the integers of bsx_resize_bgr (the 2x2 area mean at an exact factor of 2, as bsx_step_batch_vcam);
 *     convert_rgb_to_yuyv(R) if the batch asks for it.  Persistent mask and ofinal of stream s are those of bsx_step_batch_streams for that stream;
 *   - geometry: as bsx_step_batch_vcam, NOT as bsx_step_batch_mixed — any capture width, ROI and buffer alignment, and an onmask callback, are accepted;
 *   - out_w == width and out_h == height: the call IS bsx_step_batch_mixed(ids, ..., flags), with that call's own refusals (its geometry included);
 *   - n == 0: returns 0 and enqueues nothing;
 *   - BSX_EINVAL before anything is enqueued, with a bsx_last_error text naming the position and value, for: the ids errors of bsx_step_batch_streams; settings
 *     NULL with n > 0; a flag bit outside the sets above (a stream's or the batch's); a blur size that is even or above 31; a NULL d_bg on a stream that reads
 *     it; out_w or out_h <= 0; an odd out_w with BSX_STEP_YUYV; an odd capture width with BSX_STEP_YUYV_IN; d_out overlapping d_frames or any stream's background;
 *     a pending pipelined composite.  A refused call changes no state. */
BSX_API int bsx_step_batch_vcam_mixed(bsx_ctx* ctx, const int* ids, const uint8_t* d_frames, const bsx_stream_setting* settings,
                                      uint8_t* d_out, int out_w, int out_h, int n, void* stream, unsigned flags);

/* cv::resize(src, dst, Size(dw,dh)) with INTER_LINEAR on packed BGR u8 (device pointers, n images). */
BSX_API int bsx_resize_bgr(bsx_ctx* ctx, const uint8_t* d_src, int sw, int sh, uint8_t* d_dst, int dw, int dh, int n, void* stream);

/* n images, each of its own size, resized (the integers of bsx_resize_bgr) to dw x dh in ONE launch: image i is d_src [sh][sw][3] -> d_dst [dh][dw][3], device
 * pointers of any alignment (a 4-byte aligned d_dst with dw % 4 == 0 is written as whole words, any other one byte-wise; the bytes are the same).
 *   - items is a HOST array, read before the call returns; the descriptors reach the device through the staging ring of bsx_step_batch_streams (no host
 *     synchronisation unless the caller runs a ring's length ahead of the GPU), the resize tables come from the cache bsx_resize_bgr fills: one per distinct
 *     (sw, sh, dw, dh), uploaded when it is first used;
 *   - n <= n_streams of the context; n == 0 returns 0 and enqueues nothing;
 *   - the same source may appear in several items; nothing is deduplicated;
 *   - BSX_EINVAL before anything is enqueued, with a bsx_last_error text naming the position and value, for: n < 0 or n > n_streams; items NULL with n > 0; a
 *     non-positive size; a NULL d_src or d_dst; a d_dst that overlaps a source picture or another destination. */
typedef struct bsx_resize_item { const uint8_t* d_src; int sw, sh; uint8_t* d_dst; } bsx_resize_item;
BSX_API int bsx_resize_bgr_batch(bsx_ctx* ctx, const bsx_resize_item* items, int n, int dw, int dh, void* stream);

/* Video backgrounds from a decoder: n NV12 surfaces, each of its own size and pitches, resized to BGR images that each have their OWN size, in ONE kernel launch —
 * grab_background() of a video source (app/background.cc:181-190: cv::resize(raw, out, Size(width, height)) on every grab) where the frames of the background video
 * come from a hardware decoder.  What the call writes is what a `setting.d_bg` takes: a tick with video backgrounds is this call followed by
 * bsx_step_batch_surfaces (or a _geoms step).  The decoder's pool stays where it is (no two surfaces need be adjacent).
 *   - d_dst of item i is byte-identical to bsx_nv12_to_bgr(d_y, pitch_y, d_uv, pitch_uv, sw, sh, 1, tmp) followed by bsx_resize_bgr(tmp, sw, sh, d_dst, dw, dh, 1), in
 *     all three modes of the resize: proper INTER_LINEAR; the copy, where sw == dw && sh == dh; the 2x2 area mean, where both scales are exactly 2.  The surface's
 *     BGR frame is the one bsx_step_batch_surfaces defines: pixel (x, y) takes Y[y][x] and the pair UV[y >> 1][x & ~1 ..], with the integers of bsx_yuyv_to_bgr.
 *     The conversion clamps, so every tap is converted first and the resize's fixed point runs on BGR taps.  No BGR copy of the surface exists anywhere.  Bytes
 *     [sw, pitch) of a row are never read, and nothing is read beyond the last row;
 *   - the whole call is one launch, whatever the mix of source sizes, pitches and destination sizes; it takes at most BSX_MAX_GEOMS distinct (dw, dh) pairs (the
 *     grid is ragged over destination sizes: the positions are ordered by destination size on the host, stably) and any number of distinct source sizes: the table
 *     of each (sw, sh, dw, dh) comes from the cache bsx_resize_bgr fills, uploaded when it is first used;
 *   - items is a HOST array, read before the call returns; the descriptors reach the device through the staging ring of bsx_step_batch_streams (no host
 *     synchronisation unless the caller runs a ring's length ahead of the GPU);
 *   - n <= n_streams of the context; n == 0 returns 0 and enqueues nothing; the same surface may appear in several items (one video serves cameras of two sizes);
 *     works on every kind of context and asks nothing of its classes;
 *   - d_dst takes any alignment (a 4-byte aligned one with dw % 4 == 0 is stored as dwords; the bytes are the same);
 *   - BSX_EINVAL before anything is enqueued, with a bsx_last_error text naming items[i] and the offending value, for: n < 0 or n > n_streams; items NULL with
 *     n > 0; a NULL d_y, d_uv or d_dst; a plane that is not 4-byte aligned; a pitch below sw or not a multiple of 4; a non-positive or odd sw or sh; a non-positive
 *     dw or dh; any bit in flags, or a non-zero reserved; a plane of 2 GiB or more, or dw * dh * 3 >= 2^31; a ninth distinct destination size; a d_dst (dw * dh * 3
 *     bytes) that overlaps any item's Y or UV plane (its own included; a plane extends from its first byte to byte sw of its last row) or another destination.
 *     BSX_EDEVICE for a grid of 2^31 workgroups or more.  A refused call changes nothing.
 * Out of scope: BGR sources in this call (bsx_resize_bgr_batch serves them), an NV12 or YUYV destination, a bsx_background object that holds surfaces, reading an
 * NV12 background inside the step's own resize pass, and the formats P010 and I420. */
typedef struct bsx_resize_surface_item {
  const uint8_t* d_y;    /* [sh] rows of pitch_y bytes, 4-byte aligned */
  const uint8_t* d_uv;   /* [sh / 2] rows of pitch_uv bytes (U, V interleaved), 4-byte aligned */
  uint8_t* d_dst;        /* [dh][dw][3] BGR, any alignment */
  int pitch_y, pitch_uv; /* multiples of 4, >= sw */
  int sw, sh;            /* the surface: even, positive */
  int dw, dh;            /* this item's own output size: positive, any parity */
  unsigned flags;        /* 0 */
  int reserved;          /* 0 */
} bsx_resize_surface_item;   /* 56 bytes */
BSX_API int bsx_resize_surfaces_batch(bsx_ctx* ctx, const bsx_resize_surface_item* items, int n, void* stream);

/* BGR u8 [n][h][w][3] -> YUYV 4:2:2 [n][h][w][2] exactly as convert_rgb_to_yuyv (byte order Y0 V Y1 U). */
BSX_API int bsx_bgr_to_yuyv(bsx_ctx* ctx, const uint8_t* d_bgr, uint8_t* d_yuyv, int w, int h, int n, void* stream);

/* BGR u8 [n][h][w][3] -> NV12 in pitched planes, by the definition at bsx_step_batch_vcam_geoms_outs_nv12: an NV12 image is a pure function of the YUYV image
 * bsx_bgr_to_yuyv writes.  Image i's planes are at d_y + i * pitch_y * h ([h] rows of pitch_y bytes) and d_uv + i * pitch_uv * (h / 2) ([h / 2] rows of pitch_uv
 * bytes); bytes [w, pitch) of every row are not written.  The stand-alone form for callers of the other steps.  Works on a context of several classes (w, h are
 * the call's own).  BSX_EINVAL, with a bsx_last_error text, for: a NULL pointer; w, h or n not positive; an odd w or h; a pitch below w or not a multiple of 4; a
 * plane that is not 4-byte aligned.  The planes must not overlap each other or the source (not checked). */
BSX_API int bsx_bgr_to_nv12(bsx_ctx* ctx, const uint8_t* d_bgr, int w, int h, int n, uint8_t* d_y, int pitch_y, uint8_t* d_uv, int pitch_uv, void* stream);

/* NV12 in pitched planes -> BGR u8 [n][h][w][3], by the definition at bsx_step_batch_surfaces: the bytes of bsx_yuyv_to_bgr applied to the 4:2:2 image whose row y
 * repeats chroma row y / 2.  The counterpart of bsx_bgr_to_nv12 and its layout: image i's planes are at d_y + i * pitch_y * h ([h] rows of pitch_y bytes) and
 * d_uv + i * pitch_uv * (h / 2) ([h / 2] rows of pitch_uv bytes); bytes [w, pitch) of every row are not read.  d_bgr may lie at any address.  Works on a context of
 * several classes (w, h are the call's own).  BSX_EINVAL, with a bsx_last_error text, for: a NULL pointer; w, h or n not positive; an odd w or h; a pitch below w or
 * not a multiple of 4; a plane that is not 4-byte aligned.  d_bgr must not overlap the planes (not checked). */
BSX_API int bsx_nv12_to_bgr(bsx_ctx* ctx, const uint8_t* d_y, int pitch_y, const uint8_t* d_uv, int pitch_uv, int w, int h, int n, uint8_t* d_bgr, void* stream);

/* YUYV 4:2:2 (bytes Y0 U Y1 V) [n][h][w][2] -> BGR u8 [n][h][w][3], exactly cv::cvtColor(COLOR_YUV2BGR_YUYV): the conversion
 * cv::VideoCapture applies to raw camera frames for the reference (app/deepseg.cc:553, :725).  Lets a caller upload 2 B/px. */
BSX_API int bsx_yuyv_to_bgr(bsx_ctx* ctx, const uint8_t* d_yuyv, uint8_t* d_bgr, int w, int h, int n, void* stream);

/* cv::flip(src, dst, code) on packed BGR u8 [n][h][w][3] (device pointers, dst != src): code 0 flips around the x axis
 * (-v / flipVertical), code > 0 around the y axis (-h / flipHorizontal), code < 0 both (app/deepseg.cc:667-673). */
BSX_API int bsx_flip_bgr(bsx_ctx* ctx, const uint8_t* d_src, uint8_t* d_dst, int w, int h, int n, int code, void* stream);

/* cv::GaussianBlur(src, dst, Size(ksize, ksize), 0) on packed BGR u8 [n][h][w][3] (device pointers, dst != src), BORDER_REFLECT_101,
 * OpenCV's 8-bit fixed-point coefficients; ksize odd, 1 <= ksize <= 31 (the reference's default strength is 25, app/deepseg.cc:429).
 * The "blur my own room" mode of the reference = this on the camera frames, then bsx_step_batch with bg_frame_stride = one frame. */
BSX_API int bsx_gaussian_blur_bgr(bsx_ctx* ctx, const uint8_t* d_src, uint8_t* d_dst, int w, int h, int n, int ksize, void* stream);

/* n blurs, each image of its own size, its own blur size and its own pixel format, in ONE kernel launch — "every camera's background is a blur of its own frame"
 * (-p bgblur without -b, the reference's default, app/deepseg.cc:652-658) for a server whose cameras differ: the outputs are capture-size BGR images, what a
 * bsx_stream_setting's d_bg points at, so a tick in blur mode is this call followed by bsx_step_batch_geoms / bsx_step_batch_vcam_geoms (the counterpart of
 * bsx_background_grab_batch for animated backgrounds).
 *   - d_dst of item i is byte-identical to bsx_gaussian_blur_bgr(d_src, d_dst, w, h, 1, ksize); with BSX_STREAM_YUYV_IN in its flags d_src is the camera's raw YUYV
 *     4:2:2 ([h][w][2] bytes Y0 U Y1 V) and d_dst is identical to that call on the output of bsx_yuyv_to_bgr(d_src, ...) — converted as the blur reads it: no BGR
 *     copy of the frame exists anywhere;
 *   - ksize 1 is the frame itself (a copy of a BGR item, the conversion of a YUYV item), done in the same launch;
 *   - the whole call is one launch, whatever the mix of sizes, blur sizes and formats; it takes at most BSX_MAX_GEOMS distinct (w, h) pairs (the grid is ragged: the
 *     positions are ordered by size on the host, so one large image among many small ones launches no empty workgroups);
 *   - items is a HOST array, read before the call returns; the descriptors reach the device through the staging ring of bsx_step_batch_streams (no host
 *     synchronisation unless the caller runs a ring's length ahead of the GPU); the coefficient words of every blur size are uploaded once, by the first call;
 *   - n <= n_streams of the context; n == 0 returns 0 and enqueues nothing; the same source may appear in several items (one frame at two blur sizes); works on
 *     every context, a multi-class one included;
 *   - BGR items take any alignment and any size (w % 4 != 0, images smaller than the blur radius), as bsx_gaussian_blur_bgr does, up to w * h * 3 < 2^31 bytes;
 *   - BSX_EINVAL before anything is enqueued, with a bsx_last_error text naming items[i] and the offending value, for: n < 0 or n > n_streams; items NULL with
 *     n > 0; a non-positive size (or one beyond 2^31 bytes); a ksize that is even, below 1 or above 31; a NULL d_src or d_dst; a flag bit other than
 *     BSX_STREAM_YUYV_IN; a YUYV item with an odd w or a d_src that is not 4-byte aligned; a ninth distinct size; a d_dst that overlaps any source (its own
 *     included; a YUYV source extends over w * h * 2 bytes) or another destination.  BSX_EDEVICE for a grid of 2^31 workgroups or more.  A refused call changes
 *     nothing. */
typedef struct bsx_blur_item {
  const uint8_t* d_src;   /* [h][w][3] BGR, or with BSX_STREAM_YUYV_IN [h][w][2] YUYV 4:2:2 (Y0 U Y1 V) */
  uint8_t* d_dst;         /* [h][w][3] BGR */
  int w, h;
  int ksize;              /* odd, 1..31 */
  unsigned flags;         /* 0 | BSX_STREAM_YUYV_IN */
} bsx_blur_item;
BSX_API int bsx_gaussian_blur_bgr_batch(bsx_ctx* ctx, const bsx_blur_item* items, int n, void* stream);

/* The same call for NV12 decoder surfaces: n surfaces, each of its own size, pitches and blur size, blurred into capture-size BGR images in ONE kernel launch — the
 * blur mode of bsx_step_batch_surfaces, whose `setting.d_bg` takes what this call writes.  A surfaces tick in the reference's default mode is this call followed by
 * bsx_step_batch_surfaces; the decoder's pool stays where it is (no two surfaces need be adjacent) and no 3 B/px copy of a frame is made.
 *   - d_dst of item i is byte-identical to bsx_nv12_to_bgr(d_y, pitch_y, d_uv, pitch_uv, w, h, 1, tmp) followed by bsx_gaussian_blur_bgr(tmp, d_dst, w, h, 1, ksize).
 *     The surface's BGR frame is the one bsx_step_batch_surfaces defines: pixel (x, y) takes Y[y][x] and the pair UV[y >> 1][x & ~1 ..], with the integers of
 *     bsx_yuyv_to_bgr.  The frame is converted as the blur reads it: no BGR copy of the frame exists anywhere.  Bytes [w, pitch) of a row are never read;
 *   - ksize 1 is the conversion alone, done in the same launch;
 *   - the whole call is one launch, whatever the mix of sizes, blur sizes and pitches; it takes at most BSX_MAX_GEOMS distinct (w, h) pairs (the grid is ragged: the
 *     positions are ordered by size on the host, stably, so one 1920x1080 surface among many small ones launches no empty workgroup);
 *   - items is a HOST array, read before the call returns; the descriptors reach the device through the staging ring of bsx_step_batch_streams (no host
 *     synchronisation unless the caller runs a ring's length ahead of the GPU); the coefficient words are those bsx_gaussian_blur_bgr_batch uploads, once per context;
 *   - n <= n_streams of the context; n == 0 returns 0 and enqueues nothing; the same surface may appear in several items (one frame at two blur sizes); works on
 *     every kind of context, whatever its classes: blurring needs no resize table, so surfaces of classes that bsx_step_batch_surfaces refuses can still be blurred;
 *   - d_dst takes any alignment (a 4-byte aligned one with w % 4 == 0 is stored as dwords);
 *   - BSX_EINVAL before anything is enqueued, with a bsx_last_error text naming items[i] and the offending value, for: n < 0 or n > n_streams; items NULL with
 *     n > 0; a non-positive or odd w or h; a ksize that is even, below 1 or above 31; a NULL d_y, d_uv or d_dst; a plane that is not 4-byte aligned; a pitch below w
 *     or not a multiple of 4; any bit in flags; w * h * 3 >= 2^31, or a plane of 2 GiB or more; a ninth distinct size; a d_dst (w * h * 3 bytes) that overlaps any
 *     item's Y or UV plane (its own included; a plane extends from its first byte to byte w of its last row) or another destination.  BSX_EDEVICE for a grid of 2^31
 *     workgroups or more.  A refused call changes nothing.
 * Out of scope: NV12 items inside bsx_gaussian_blur_bgr_batch, an NV12 or YUYV destination, blur as a bit of bsx_surface_item.setting, and the formats P010 and
 * I420 (three planes) as sources. */
typedef struct bsx_blur_surface_item {
  const uint8_t* d_y;    /* [h] rows of pitch_y bytes, 4-byte aligned */
  const uint8_t* d_uv;   /* [h / 2] rows of pitch_uv bytes (U, V interleaved), 4-byte aligned */
  uint8_t* d_dst;        /* [h][w][3] BGR, any alignment */
  int pitch_y, pitch_uv; /* multiples of 4, >= w */
  int w, h;              /* even, positive */
  int ksize;             /* odd, 1..31 */
  unsigned flags;        /* 0 */
} bsx_blur_surface_item;   /* 48 bytes */
BSX_API int bsx_gaussian_blur_surfaces_batch(bsx_ctx* ctx, const bsx_blur_surface_item* items, int n, void* stream);

/* ---- background source (app/background.cc) ----
 * load_background(): a still image or an animation (GIF87a/89a, 8-bit non-interlaced PNG, binary PPM decoded in this library; other
 * formats through bsx_background_from_frames with frames the caller decoded).  The frames live on the context's GPU; an animation gets
 * the FPS-paced reader thread of background.cc:29-104 (advances one frame per 1/fps, wraps to 0 at the end).  NULL on error. */
typedef struct bsx_background bsx_background;
BSX_API bsx_background* bsx_background_load(bsx_ctx* ctx, const char* path, int debug);
BSX_API bsx_background* bsx_background_from_frames(bsx_ctx* ctx, const uint8_t* h_bgr, int width, int height, int n_frames, double fps, int debug);
BSX_API void bsx_background_free(bsx_background* bg);
BSX_API int bsx_background_info(const bsx_background* bg, int* width, int* height, int* n_frames, double* fps, int* is_video);
/* grab_background(): the current frame resized (cv::resize INTER_LINEAR) to width x height into d_bgr_out [height][width][3].
 * Returns the frame number or -1 on error: 1 for a still image; for an animation the reference's count of pictures read since the last rewind, i.e.
 * picture c (= floor(t * fps) mod n, t since the background was created: real-time playback, looping at the end) is reported as c + 1. */
BSX_API int bsx_background_grab(bsx_background* bg, int width, int height, uint8_t* d_bgr_out, void* stream);
/* grab_background() for n sources at once, in ONE launch (bsx_resize_bgr_batch): output i = the current picture of bgs[i] resized to width x height, at
 * d_bgr_out + i * out_stride — what a bsx_stream_setting's d_bg points at, grabbed every tick (out_stride a multiple of 4 keeps every slice 4-byte aligned).
 *   - at_seconds >= 0: picture floor(at_seconds * fps_i) mod n_i of every animation (a still is always its one picture) — "the backgrounds as of tick t", the
 *     same for every caller and every run; at_seconds < 0: the clock, read ONCE for the whole batch (t_i = now - creation of bgs[i], as bsx_background_grab);
 *   - frame_nos (host, may be NULL): entry i = what bsx_background_grab would have returned for it (1 for a still, picture c as c + 1);
 *   - bgs and frame_nos are host arrays, read / written before the call returns; the same source may appear in several entries (a caller who wants one output
 *     shared by many streams lists it once and points those settings at it); n <= n_streams of the sources' context; n == 0 returns 0 and enqueues nothing;
 *   - returns 0, or BSX_EINVAL before anything is enqueued — the text, naming the position and value, is bsx_last_error of the sources' context and of
 *     bsx_last_error(NULL) — for: n < 0 or n > n_streams; bgs NULL with n > 0, a NULL entry, an entry of another context than bgs[0]'s; a non-positive size; a NULL
 *     d_bgr_out; out_stride < width * height * 3; at_seconds NaN or infinite; an output that overlaps the pictures of a source.  A refused call writes no
 *     frame_nos. */
BSX_API int bsx_background_grab_batch(bsx_background* const* bgs, int n, int width, int height, uint8_t* d_bgr_out, size_t out_stride, double at_seconds,
                                      int* frame_nos, void* stream);
/* host-only decode of the same formats (no GPU): frames → malloc'ed [n][h][w][3] BGR; returns n (> 0) or a negative BSX_E* code */
BSX_API int bsx_media_decode(const char* path, int* width, int* height, double* fps, uint8_t** h_bgr, char* errbuf, size_t errcap);
BSX_API void bsx_media_free(uint8_t* h_bgr);

/* ---- live single-camera mode: class CalcMask (app/deepseg.cc:159-286) ----
 * set_input_frame clones the frame into pinned memory and enqueues upload + mask pipeline (stream slot 0) + mask download on a private HIP
 * stream; it never waits for the GPU (up to two submissions in flight; a frame that finds both busy replaces the one already waiting).
 * get_output_mask polls the completion events: it copies the newest finished mask (returns 1) or leaves h_mask untouched (0).
 * timings: how long the queue sat idle before the last submission / upload + pipeline + download of the last mask handed out (HIP events). */
typedef struct bsx_live bsx_live;
BSX_API bsx_live* bsx_live_new(bsx_ctx* ctx);
BSX_API void bsx_live_delete(bsx_live* live);
BSX_API int bsx_live_set_input_frame(bsx_live* live, const uint8_t* h_bgr, size_t bgr_stride);
BSX_API int bsx_live_get_output_mask(bsx_live* live, uint8_t* h_mask, size_t mask_stride);
BSX_API int bsx_live_timings(const bsx_live* live, long* waitns, long* loopns);

/* ---- introspection used by the parity tests and the bench (stage-by-stage checks) ---- */
/* Device pointer + element count of: 0 = model input tensor [n_streams][in_h][in_w][in_c] f32,
 * 1 = model output tensor f32, 2 = ofinal u8 [n_streams][out_h][out_w], 3 = masks u8,
 * 4 = the 8-bit network input the steps' prep writes, [n_streams][in_h][in_w] 32-bit words R | G<<8 | B<<16, indexed by POSITION in the call (a multi-geometry
 *     call orders its positions by class, the caller's order kept within a class); BSX_EINVAL where the stem reads the f32 form (0) instead. */
BSX_API int bsx_debug_buffer(bsx_ctx* ctx, int which, void** d_ptr, size_t* bytes);
/* Run single stages on the current buffers (n streams): 0 = prep, 1 = infer, 2 = decode+IIR, 3 = upscale+blur, 4 = prep on raw YUYV 4:2:2 frames
 * (BSX_STEP_YUYV_IN's form of stage 0; BSX_EINVAL where the fused form does not apply). */
BSX_API int bsx_debug_run_stage(bsx_ctx* ctx, int stage, const uint8_t* d_frames, int n, void* stream);
/* Per-launch description of the fused plan, one line per GPU launch; returned string is owned by ctx. */
BSX_API const char* bsx_plan_describe(bsx_ctx* ctx);
/* Copy out the value of graph tensor `tensor_idx` for stream 0 after an infer; returns element count or negative error.  h_out may be NULL to query the size.
 * Only tensors that the executing path writes to HBM are served: a tensor that the planner fused away, that the frame program keeps in LDS or elides, or that
 * lives inside a fused launch is refused with BSX_EINVAL, and bsx_last_error names the reason.  A tensor that the path stores as packed halves (arena activations
 * under BSX_ACT16, the fused blocks' depthwise outputs under BSX_F16_GEMM=fast16 from 8192 rows of the last network stage) is served widened to f32.
 * Indices from the file's tensor count upwards name the tensors a graph rewrite created (a 1x1 convolution moved below its resize stores one where the file has
 * none; the plan text shows them as the `t<idx>` of the rewrite's steps): served under the same rule, BSX_EINVAL past the last of them.
 * Without the debug build's BSX_ARENA_NO_REUSE a served tensor's arena slot may since have been reused by a later step. */
BSX_API long bsx_debug_tensor(bsx_ctx* ctx, int tensor_idx, float* h_out, long cap);
/* The same for stream `stream_idx` of the last batch (full-batch parity tests: every stream against its twin). */
BSX_API long bsx_debug_tensor_of(bsx_ctx* ctx, int tensor_idx, int stream_idx, float* h_out, long cap);

/* How the fused mask + blend launch would classify its tiles for the CURRENT temporal state of the first n streams (host-side, exact same extents as the kernel):
 * out4 = {tiles, tiles whose whole source block is 0xFF, ... 0x00, tiles on the general path}.  A uniform tile skips the up-scale / blur phases and reads only the
 * operand its composite is a copy of (kernels_img.hip: mask_tile_k); bench.py uses the counts to state the bytes the launch really has to move. */
BSX_API int bsx_debug_mask_tile_stats(bsx_ctx* ctx, int n, long* out4);

/* Per-frame-program timeline: runs the network once for n streams and returns, for workgroup 0, the wall-clock
 * (100 MHz constant-rate counter) ticks at the start of every micro-op plus one final tick; ticks[i+1]-ticks[i] = op i.
 * Returns the number of micro-ops (cap must be >= that + 1), 0 if the program path is off, negative on error. */
BSX_API int bsx_debug_program_timeline(bsx_ctx* ctx, int n, unsigned long long* ticks, int cap, void* stream);

/* Host only, no GPU: the coefficient words gauss_blur_k multiplies with for cv::GaussianBlur(ksize, sigma 0) on 8-bit images (app/deepseg.cc:657-658) when its LDS
 * planes start `shift` (0..3) pixels left of the tile — c4[4][9]: the u8 taps packed 4 per word, delayed by j + shift bytes for output phase j; c2[2][17]: the same taps
 * as u16 pairs delayed by h halves.  The parity tests check them against the oracle's taps (the kernels' arithmetic is only as right as these tables).  Returns 0 or BSX_EINVAL. */
BSX_API int bsx_debug_gauss_coeffs(int ksize, int shift, uint32_t* c4 /* 36 */, uint32_t* c2 /* 34 */);

/* Parse a .tflite file and build the fused plan WITHOUT touching a GPU; writes a text description
 * ("ops=<n> nodes=<n> steps=<n> macs=<per frame> arena_floats=<per stream>" then one line per launch)
 * into buf (NUL-terminated, truncated to cap).  Returns 0, or BSX_EMODEL with the reason in buf. */
BSX_API int bsx_model_describe(const char* model_path, char* buf, size_t cap);
/* Host only, no GPU: build the plan of `model_path`, emit the kernel specialised to that graph (the per-frame program of the Meet / MLKit
 * family as straight-line code: csrc/gen_mid.cpp) and compile it with hipRTC for `arch` (NULL = "gfx950") into the code-object cache, so
 * that bsx_new on the GPU box only loads it — and the same for the graph's segment kernels (csrc/gen_seg.cpp).  This replaces what InterpreterBuilder / AllocateTensors do when the reference creates its
 * context (lib/libbackscrub.cc:205-217).  msg receives "compiled" / "cached" / why the graph stays interpreted.  Returns 0, or BSX_EMODEL. */
BSX_API int bsx_model_precompile(const char* model_path, const char* arch, char* msg, size_t cap);
/* The generated source itself (tests, inspection): returns its length (without NUL), copies at most cap - 1 bytes; 0 when the graph has no
 * specialised form (reason in buf), negative on a model error. */
BSX_API long bsx_model_kernel_source(const char* model_path, char* buf, size_t cap);
/* The same for the SEGMENT kernels of the graph (csrc/gen_seg.cpp: the high-resolution ends of the Meet / MLKit networks — the source of csrc/kernels_seg.hip with this
 * plan's descriptors and template arguments as compile-time constants; bsx_model_precompile compiles it next to the program's kernel, bsx_new loads it). */
BSX_API long bsx_model_seg_source(const char* model_path, char* buf, size_t cap);

/* ---- measurement ---- */
typedef struct bsx_launch_stat {
  char name[64];      /* kernel / fused step label */
  double avg_ms;      /* mean duration of this launch over `iters` repetitions: from the hipEvent behind the launch in front of it to the one behind itself */
  double bytes;       /* ALGORITHMIC bytes this launch must move for n streams (inputs once + outputs once) */
  double flops;       /* 2*MAC for n streams (0 for byte kernels) */
} bsx_launch_stat;

/* Runs the whole per-batch sequence (prep, every fused network step, decode, upscale+blur, blend)
 * `iters` times with ONE hipEvent on `stream` between consecutive launches (the per-launch figures add up to the pass), and writes one record per
 * launch (in launch order) into out[0..cap).  Returns the number of launches, or a negative error.
 * The temporal state advances exactly as `iters` calls of bsx_step_batch would. */
BSX_API int bsx_profile_batch(bsx_ctx* ctx, const uint8_t* d_frames, const uint8_t* d_bg, size_t bg_frame_stride, uint8_t* d_out,
                      int n, int iters, bsx_launch_stat* out, int cap, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* BSX_H_ */
