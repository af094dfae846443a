/* ks265_enc.h — the library boundary "B2" of SURVEY.md §8(b): the encoder API of the KSC265 SDK (qy265enc.h:196-233, qy265def.h:7-22,
 * 179-198 under /root/reference/Android_demo/prebuilt/include/), served by the MI355X pixel path + the host bitstream writer.
 *
 * A caller written against the SDK keeps including the SDK's own qy265enc.h / qy265def.h and links libks265enc.so instead of libqyencoder:
 * the entry points have the SDK's names and signatures, the structures below have the SDK's layout (field order and types; checked
 * against offsets computed from the SDK header by tests/test_enc_api.py).  This header exists so that the library, its CLI and its tests
 * compile without the SDK; its comments say what THIS implementation does with each field.
 *
 * Behaviour that differs from the SDK, all of it reported through the log callback at open:
 *   - the encoder's decisions are its own: the stream is a conforming HEVC stream, not appencoder's bytes;
 *   - rate control: rc = 0 is constant QP with the reference's own hidden ladders (read from its -psnr 2 lines): I = Q; IPPP P pictures
 *     Q + 1 + {0, 2, 1, 2}[position & 3]; hierarchical GOP anchors Q + 1, B layers Q + 2 / + 4 / + 4 (-bframes 3, a pyramid of 4: Q + 2 / + 3); P + n plain B: B = Q + 2 (-fixqp 1: one QP);
 *     rc = 3 (CRF) maps crf to that ladder; rc = 1 / 2 / 4 (bitrate targets) run a frame-level controller on top of it (one offset per
 *     mini-GOP from the pictures coded so far: deterministic streams); rc = 5 and VBV are not implemented;
 *   - subme 0 / 1 / 2 and the preset's thresholds run the reference's sub-pel refinement (include/ks265_hip.h ks265_frame_cfg.subme);
 *   - part = 1 codes 2NxN / Nx2N prediction units (CUs of 64 / 32 / 16 samples; priced with the vectors of the square search);
 *     iAqMode / fAqStrength (-aq / -aqs) give every CTU its own QP (cu_qp_delta) from the reference's calcFrameAdaptQuant arithmetic;
 *   - lookahead: with the default hierarchical GOP (bframes -1 / 7) the slice-type decision (a block of 8 pictures coded as 8 or as 4 + 4)
 *     runs by itself, so the GOP layout depends on the content unless lookahead = 0; lookahead N > 0 adds scene-cut key pictures;
 *   - refnum with the pyramid GOPs gives the B pictures up to 4 reference pictures per list (round 5); ref0 (round 6; every preset from superfast up resolves to 3) gives the
 *     anchors of a pyramid the last ref0 anchors of their GOP to search; tuInter >= 1 codes 2Nx2N inter CUs of 32 / 16 samples with four transform units where the residual sits
 *     in part of the CU (one level of the residual quadtree; deeper values run as 1);
 *   - rdoq (round 6): the presets' rdoq = 1 runs this build's own seam (dead zone, coefficient-group pruning, sign-data hiding); rdoq set BY NAME (QY265ConfigParse "rdoq" "1" =
 *     `-rdoq 1`, stored as 2) sends the luma transform blocks of inter CUs through the reference's rdoQuant with bit tables that follow the stream; "0" = the seam;
 *   - sao: every level > 0, the presets' 3 (veryfast, fast) included, = this build's rule over all four edge classes + band offset; sao 3 set BY NAME (QY265ConfigParse "sao" "3" =
 *     `-sao 3`, stored as 5) = the reference's decision on its -sao 4 path (band offset + the 0 / 90 degree edge classes, its estimation functions, rates and lambda table, no merge
 *     candidates) - measured on configs[0]: 5.5 % more bytes at equal PSNR-Y than the build's rule, which is why the presets do not select it;
 *   - sao-ref (not in the SDK; QY265ConfigParse "sao-ref" = `-sao-ref`): the reference's decision under a name of its own - "1" = what sao 3 by name selects (stored as 5),
 *     "2" = the same with the reference's merge candidates (stored as 6): a CTU whose left or upper CTU's final parameters are strictly cheaper on its own statistics takes
 *     them and codes sao_merge_left_flag / sao_merge_up_flag instead of its parameters; "0" leaves sao as it is.  No preset selects it;
 *   - calcSsim (-ssim 1 | 2): the reference's ` ssim:` line behind `bitrate, psnr:` (8x8 windows), computed on the device in the same pass as the SSE; 2 adds one
 *     `ks265enc: poc N ssim Y U V` line per picture (the reference prints nothing per picture); totals and the last picture's values: ks265_enc_get_quality;
 *   - hash (not in the SDK; ks265_enc_set_default "hash" = `-hash N`, below): a decoded picture hash SEI message behind every picture, CRC or checksum, computed on the device;
 *   - vpp_denoise (0 off, 1 gentle, 2 medium, 3 aggressive; QY265ConfigParse "denoise" = `-denoise N`) and vpp_recur_filter (0 .. 30; "recur" = `-recur V`): a motion-compensated
 *     temporal filter on the GPU, the last step a picture takes on its way in - behind the upload, the conversion, the scaler or the padding, in the caller's stream order, for
 *     host pictures, acquired slots and device pictures alike (tests/denoise_ref.py is the specification of every byte).  Per 16x16 luma block of the coded
 *     picture an exhaustive integer search (+-8) in the previous FILTERED picture; a block that matches (SAD below thr per sample) is blended towards its prediction, sample by
 *     sample, by a weight that falls from weight / 32 to 0 as the difference grows to thr; one that does not stays as it is.  Levels 1 / 2 / 3 = (thr, weight) (6, 16) /
 *     (10, 20) / (16, 24); vpp_recur_filter v > 0 replaces the weight by round(v), at least 1, and alone runs at thr 10.  These values are this build's choice (the reference's
 *     Linux binaries have no VPP code); they were tried on synthetic noise only.  Everything downstream - the lookahead, the search, `analysis`, `devrecon`, -o - sees the
 *     filtered picture, and -psnr / -ssim are measured AGAINST THE FILTERED PICTURE, as they are against the scaled one.  History: a lane's first picture has none, and neither
 *     has the first picture of a GOP chunk dealt to a lane; a one-lane handle never restarts, the recursion runs across its periodic key pictures.  With several GOP lanes every
 *     chunk therefore starts unfiltered and the stream differs between lane counts: the known limit - history is not carried between lanes or GPUs.  QY265EncoderReconfig
 *     leaves the filter as opened.  Values outside the ranges, or a device library without ks265_input_denoise: QY265EncoderOpen fails with QY_NOTSUPPORTED.  Both 0 (the
 *     default): no call, no allocation, no byte of the stream changes;
 *   - vpp_edge and vpp_color (each 0 off, 1 gentle, 2 medium, 3 aggressive; QY265ConfigParse "edge" = `-edge N`, "color" = `-color N`): edge and colour enhancement on the GPU,
 *     one stateless step behind the denoiser and in front of the encoder, for every way in (tests/enhance_ref.py is the specification of every byte).  Luma: an
 *     unsharp mask - the detail against the exact 5x5 binomial blur, cored (a soft threshold), amplified, limited, added, and the result held inside the sample's 3x3
 *     neighbourhood's minimum / maximum widened by `over` (halo control); picture edges replicate.  Levels 1 / 2 / 3 = (gain in 1/16, core, limit, over) (8, 2, 8, 2) /
 *     (16, 2, 16, 4) / (24, 3, 24, 8).  Chroma: every (u, v) pair is pushed away from grey by a gain that falls linearly from 1 + g / 64 at grey to 1 at full saturation
 *     (g = 8 / 16 / 32); grey stays grey, nothing clips.  These values are this build's choice (the reference's Linux binaries have no VPP code) and NOBODY HAS TRIED THEM ON
 *     REAL FOOTAGE.  The range that goes in is not protected: a limited-range picture may leave 16 .. 235 by `over`.  With the denoiser on, its history stays unsharpened: the
 *     recursion never sees enhanced samples.  The filter has no state, so any number of GOP lanes gives the one-lane stream.  Everything downstream - the lookahead, -aq, the
 *     search, `analysis`, `devrecon`, -o - sees the enhanced picture, and -psnr / -ssim are measured AGAINST THE ENHANCED PICTURE.  QY265EncoderReconfig leaves the filter as
 *     opened.  Values outside 0 .. 3, or a device library without ks265_input_enhance: QY265EncoderOpen fails with QY_NOTSUPPORTED.  Both 0 (the default): no call, no
 *     allocation, no byte of the stream changes;
 *   - vpp_hdr (0 / 1; QY265ConfigParse "hdr" = `-hdr 0|1`) with vpp_hdr_strength (0 .. 5; "hdr-strength"), vpp_hdr_iter (2 or 3; "hdr-iter"), vpp_hdr_sigma_s and vpp_hdr_sigma_r
 *     (each 0 .. 100; "hdr-sigma-s", "hdr-sigma-r"; sigma_r a percentage of the 8-bit range): local contrast on the GPU, one stateless step between the denoiser and the
 *     enhancement, for every way in (tests/hdr_ref.py is the specification of every byte).  Luma only: the base layer is vpp_hdr_iter iterations of the domain
 *     transform in its normalised-convolution form - rows, then columns, the radius halved each iteration, guided by the luma that came in, exact in integers - and the
 *     result is Y + strength (Y - base), rounded and clipped: contrast at large scale, no halo at a strong edge.  No tone curve on the base; chroma is not touched.  A field
 *     left at 0 takes this build's default - strength 1.0, iter 3, sigma_s 20, sigma_r 15 = (gain 16/16, slope 8, radii 484 / 242 / 121 in 1/16 sample).  These values are
 *     this build's choice (the reference's Linux binaries have no VPP code) and NOBODY HAS TRIED THEM ON REAL FOOTAGE.  The range that goes in is not protected.  The
 *     denoiser's history never sees boosted samples; with vpp_edge on, the enhancement then reads a luma copy of its own.  The filter has no state, so any number of GOP
 *     lanes gives the one-lane stream.  Everything downstream - the lookahead, -aq, the search, `analysis`, `devrecon`, -o - sees the filtered picture, and -psnr / -ssim are
 *     measured AGAINST THE FILTERED PICTURE.  QY265EncoderReconfig leaves the filter as opened.  vpp_hdr other than 0 / 1, a field outside its range, or a device library
 *     without ks265_input_hdr: QY265EncoderOpen fails with QY_NOTSUPPORTED.  vpp_hdr 0 (the default): the other four fields are not looked at; no call, no allocation, no
 *     byte of the stream changes;
 *   - transskip, tuIntra, 2-pass, long-term references, VBV / CVQ: accepted, ignored;
 *   - input pictures: the caller's planes are pinned in place and uploaded from where they lie inside QY265EncoderEncodeFrame; the caller may reuse its buffers when the call returns
 *     (the SDK requires them to stay valid until the frame is done);
 *   - analysis out (not in the SDK; ks265_enc_set_default "analysis", ks265_enc_get_device_analysis below): motion, modes, QP and block error of every picture as device arrays;
 *   - reconstructed pictures in device memory (not in the SDK; ks265_enc_set_default "devrecon", ks265_enc_get_device_recon below): I420, NV12 or RGB(A), in the caller's stream order;
   - pictures in device memory (not in the SDK): ks265_enc_encode_device_frame takes I420, NV12 or RGB(A) planes on the GPU and converts them there, in the caller's stream
 *     order (ks265_dev_picture below) - no host copy, no upload, no pinning.
 */
#ifndef KS265_ENC_H
#define KS265_ENC_H
#ifdef __cplusplus
extern "C" {
#endif

/* qy265def.h:7-22 */
enum { QY_OK = 0, QY_FAIL = (int)0x80000001, QY_OUTOFMEMORY = (int)0x80000002, QY_POINTER = (int)0x80000003, QY_NOTSUPPORTED = (int)0x80000004,
       QY_AUTH_INVALID = (int)0x80000005 };

typedef enum QY265Tune_tag { QY265TUNE_DEFAULT = 0, QY265TUNE_SELFSHOW, QY265TUNE_GAME, QY265TUNE_MOVIE, QY265TUNE_SCREEN } QY265Tune;
typedef enum QY265Preset_tag { QY265PRESET_ULTRAFAST = 0, QY265PRESET_SUPERFAST, QY265PRESET_VERYFAST, QY265PRESET_FAST, QY265PRESET_MEDIUM, QY265PRESET_SLOW,
                               QY265PRESET_SLOWER, QY265PRESET_VERYSLOW, QY265PRESET_PLACEBO } QY265Preset;
typedef enum QY265Latency_tag { QY265LATENCY_ZERO = 0, QY265LATENCY_LOWDELAY, QY265LATENCY_LIVESTREMING, QY265LATENCY_DEFAULT } QY265Latency;

/* qy265enc.h:51-148, same field order and types */
typedef struct QY265EncConfig {
    void *pAuth;                              /* ignored (no licence check) */
    QY265Tune tune; QY265Preset preset; QY265Latency latency;
    int profileId;                            /* 1 = Main (the only one written) */
    int bHeaderBeforeKeyframe;                /* VPS / SPS / PPS in front of every key picture */
    int picWidth, picHeight;                  /* even (PICTURE SIZES below: a size that is no multiple of 8 is coded with a conformance window) */
    double frameRate;
    int bframes;                              /* -1: preset / latency default (hierarchical GOP 8 at default latency, else 0); 0: IPPP; 3 / 7: pyramids of 4 / 8 as in the reference; other n: n non-reference B pictures per anchor (at most 16: more is QY_NOTSUPPORTED at open) */
    int temporalLayer;
    int vpp_denoise, vpp_edge, vpp_color, vpp_hdr; double vpp_hdr_strength; int vpp_hdr_iter; double vpp_hdr_sigma_s, vpp_hdr_sigma_r, vpp_recur_filter;
    int rc;                                   /* 0 CQP, 1 CBR, 2 ABR, 3 CRF, 4 CVBR, 5 CVQ */
    int bitrateInkbps, vbv_buffer_size, vbv_max_rate, vbv_min_rate;
    int qp, crf, visual_quality;
    int iIntraPeriod;                         /* key picture (IDR) period, -1 = only the first */
    int qpmin, qpmax, enFrameSkip;
    int enWavefront, enFrameParallel;         /* the GPU path is frame-wide; ignored */
    int threads;                              /* host threads writing slice data (one picture each), 0 = all cores */
    int vui_parameters_present_flag;
    struct { int video_signal_type_present_flag, video_format, video_full_range_flag, colour_description_present_flag, colour_primaries,
             transfer_characteristics, matrix_coeffs; } vui;
    int logLevel, lookahead, calcPsnr, calcSsim, shortLoadingForPlayer;
    int iPass; char statFileName[256]; double fRateTolerance;
    int rdoq, me, part, do64, tuInter, tuIntra, smooth, transskip, subme, satdInter, satdIntra, searchrange, refnum, ref0, sao, longTermRef, iAqMode;
    double fAqStrength;
    int rasl;
} QY265EncConfig;

/* qy265enc.h:160-184 */
typedef struct QY265YUV { int iWidth, iHeight; unsigned char *pData[3]; int iStride[3]; } QY265YUV;
typedef struct QY265Picture { int iSliceType; int poc; long long pts; long long dts; QY265YUV *yuv; } QY265Picture;
typedef struct QY265Nal { int naltype; int tid; int iSize; long long pts; unsigned char *pPayload; } QY265Nal;

typedef void (*QYLogPrintf)(const char *msg);
void QY265SetLogPrintf(QYLogPrintf cb);                       /* qy265def.h:188; NULL = stdout */
extern const char strLibQy265Version[];                        /* qy265def.h:198 */

void *QY265EncoderOpen(QY265EncConfig *pCfg, int *errorCode);  /* NULL + *errorCode on failure */
void QY265EncoderClose(void *pEncoder);
void QY265EncoderReconfig(void *pEncoder, QY265EncConfig *pCfg);          /* qp / bitrate / iIntraPeriod take effect at the next picture */
int QY265EncoderEncodeHeaders(void *pEncoder, QY265Nal **pNals, int *iNalCount);
/* pInpic == NULL flushes.  The NAL array and payloads belong to the encoder and stay valid until the next call.  Returns QY_OK or an error. */
int QY265EncoderEncodeFrame(void *pEncoder, QY265Nal **pNals, int *iNalCount, QY265Picture *pInpic, QY265Picture *pOutpic, int bForceLogo);
void QY265EncoderKeyFrameRequest(void *pEncoder);
int QY265EncoderDelayedFrames(void *pEncoder);
int QY265ConfigDefault(QY265EncConfig *pConfig, QY265Preset preset, QY265Tune tune, QY265Latency latency);
int QY265ConfigDefaultPreset(QY265EncConfig *pConfig, char *preset, char *tune, char *latency);
#define QY265_PARAM_BAD_NAME (-1)
#define QY265_PARAM_BAD_VALUE (-2)
int QY265ConfigParse(QY265EncConfig *p, const char *name, const char *value);

/* not in the SDK: totals of the session for the CLI's summary lines */
typedef struct { long frames; long long bytes; double sse[3]; double gpu_ms; double host_write_ms;
                 double in_copy_ms, submit_ms, output_ms;   /* calling thread: input copy to pinned memory, enqueueing GPU work, waiting for / copying output */
                 double lat_gpu_ms, lat_queue_ms;           /* summed per picture: enqueue -> records on the host; enqueue -> a writer thread picked the picture up */
                 double key_wall_ms, key_cpu_ms; long keys; /* key pictures: records on the host -> slice finished (wall), summed thread time of its rows */
                 long occ_samples, occ_ring, occ_gpu, occ_ready;   /* sampled at every submission: pictures in the ring, of them not yet through the GPU, of them waiting for a writer */
                 double submit_wait_ms;                     /* the part of submit_ms the scheduler thread spent WAITING for a free ring slot (not runtime calls) */
} ks265_enc_stats;
int ks265_enc_get_stats(void *pEncoder, ks265_enc_stats *out);
/* not in the SDK: the quality figures of the pictures handed out so far (accounted in output order, so the totals are the same for any number of GOP lanes).
 * sse: summed squared error per plane (calcPsnr != 0, else 0; = ks265_enc_stats.sse).  ssim: per plane the SUM over the pictures of the picture's SSIM as the reference's
 * `-ssim` computes it (calcSsim != 0 and a device library that has the pass: have_ssim, else 0) - the ` ssim:` line prints ssim[k] / frames.
 * last_*: the picture accounted last (its display index in the stream - with GOP lanes in its GOP - and its own SSE and SSIM values; last_poc = -1 before the first). */
typedef struct { long frames; int have_sse, have_ssim; double sse[3]; double ssim[3]; int last_poc; double last_sse[3]; double last_ssim[3]; } ks265_enc_quality;
int ks265_enc_get_quality(void *pEncoder, ks265_enc_quality *out);
/* extension: closed GOPs coded concurrently by this handle ("GOP lanes": KS265_GOP_LANES = 2..4 with enFrameParallel, -rc 0, key period >= 32, any GOP structure;
 * default: 2 for the pyramid GOPs - the SDK's default GOP and -bframes 3 - on one GPU with -rc 0 / -rc 3, where lanes leave the stream as it is (round 5: their B pictures leave the device under-filled, two closed GOPs side by side
 * code 700 pictures/s where one codes 631 at 2160p), 1 otherwise; KS265_GOP_LANES=1 switches it off).  Output stays in stream order and is byte for byte the one-lane stream;
 * it lags the input by up to that many GOPs, and every lane buffers a GOP of input (pinned host memory + a device twin per picture, capped by KS265_PINNED_MB per lane). */
int ks265_enc_lanes(void *pEncoder);
/* extension: the switches of the reference CLI that QY265EncConfig has no field for - "df" (deblocking, default 1), "fixqp" (1 = no per-layer QP offsets: every
 * picture at -qp), "md5" (1 = log `POC n MD5 y,u,v` of every reconstructed picture, display order).  Process-wide defaults read by the next QY265EncoderOpen.
 * "gpb" (0 / 1, default 0; other values QY265_PARAM_BAD_VALUE; the environment's KS265_GPB=0|1 overrides it at QY265EncoderOpen; `ks265enc -gpb N`): generalised B anchors, as the
 * reference codes them (its -psnr 2 lines show every anchor of the pyramid as a B slice).  An anchor of a GOP with B pictures takes the pictures it takes anyway - the last
 * min(-ref0, anchors since the key picture) anchors of its GOP, a1 nearest, the key picture counting - and with
 *     one of them   stays the P slice on [a1] it is;
 *     two           goes out as a B slice with list 0 = [a1], list 1 = [a2];
 *     three / four  as a B slice with list 0 = [a1, a3(, a4)], list 1 = [a2]
 * (no picture in both lists; bi-prediction pairs the two nearest anchors; every picture is searched once).  Reference picture sets, DPB size and NAL types stay; the lists are not
 * the default construction, so the stream's PPS carries lists_modification_present_flag = 1 where the switch is in force.  Such a picture remains an anchor to everything else:
 * QP ladder and lambda, rate control, lookahead / cuTree, scene cuts, -aq, GOP lanes; it keeps the full tool set and runs without the skip pass like a P picture.
 * QY265Picture.iSliceType and the -psnr 2 lines report it as the stream does: B.  The switch is accepted and does nothing where no anchor searches two anchors: -bframes 0,
 * zero latency, -ref0 1, and P + n plain B pictures (whose anchors keep one reference); there the stream is byte for byte the one without it.  Measured: DESIGN.md 5d. */
/* "hash" (x265's numbering: 0 = off, the default; 2 = CRC; 3 = checksum; the environment's KS265_HASH overrides it at QY265EncoderOpen; `ks265enc -hash N`): every coded picture
 * is followed by a suffix SEI NAL unit (type 40) with its decoded picture hash message (H.265 D.2.19 / D.3.19, payload type 132; hash_type 1 = picture_crc, 2 =
 * picture_checksum of the three planes of the output picture), so that any decoder can verify its output against this encoder's reconstruction.  1 (MD5) and every other value:
 * QY265_PARAM_BAD_VALUE - MD5 is sequential over a plane, which means the whole picture on the host and one thread hashing it; that remains what "md5" does, for log lines.
 * CRC and checksum are computed by one kernel launch that reads the output picture once (ks265_picture_hash); 24 bytes come home per picture.  The switch works
 * with GOP lanes and several GPUs (the message travels with its picture; any number of lanes gives the same bytes) and does not bring the reconstruction to the host.
 * QY265EncoderEncodeFrame hands the message out as one more QY265Nal (naltype 40) behind the picture's, with its pts.  ks265_enc_stats.bytes and the bitrate lines count it; the
 * rate controllers and the -rdoq tables do not: for every -rc mode the stream minus its type-40 NAL units is byte for byte the stream without the switch.  On a device library
 * without the pass the encoder logs `ks265enc: picture hash is unavailable: ...` once and writes no messages. */
int ks265_enc_set_default(const char *name, int value);
/* extension: zero-copy input.  Fills `yuv` with the planes of one of the encoder's pinned input buffers (packed I420, strides = width, width / 2); the caller writes the
 * next picture there and passes the same QY265YUV to QY265EncoderEncodeFrame, which then copies nothing (0.35 ms of the calling thread per 2160p picture otherwise).
 * Never blocks: QY_FAIL when no buffer is free at the moment - pass your own buffer then, it is copied as usual.  At most one buffer is out at a time.
 * CONTRACT: the buffer belongs to the caller only until the NEXT QY265EncoderEncodeFrame call on this handle, whatever picture that call hands in - if it hands in another
 * buffer and no free input slot is left, the encoder copies that picture into the acquired buffer (its last resort; anything the caller had written there is lost).  Acquire,
 * fill and hand in the same buffer, one picture at a time.  With the lookahead every input slot also has a twin in device memory (picture size each; logged at open). */
int ks265_enc_acquire_input(void *pEncoder, QY265YUV *yuv);
/* extension: pictures in device memory.  ks265_enc_enable_device_input (between Open and the first picture; QY_NOTSUPPORTED after it, for a handle whose GOP lanes span several
 * GPUs, and with the KS265_GRAPH experiment) gives every input slot a twin in device memory; from then on ks265_enc_encode_device_frame takes pictures whose planes lie on `device`
 * (the handle's GPU: else QY_NOTSUPPORTED), as QY265EncoderEncodeFrame takes host pictures - the same key requests, GOP lanes, delayed frames, zero latency and output; both
 * kinds of picture may be mixed.  Each plane must lie inside one device allocation of the HIP runtime on that device, [plane, plane + pitch (rows - 1) + row bytes): else
 * QY_POINTER, and nothing is enqueued (host, managed and other devices' memory, short buffers, pitches below the row).  Width a multiple of 8 as for the encoder.
 *   KS265_IN_I420  plane[0..2] = Y, U, V with their own pitches;  KS265_IN_NV12  plane[0] = Y, plane[1] = interleaved UV (height / 2 rows);
 *   KS265_IN_RGB   plane[0..2] = the R, G, B samples of pixel (0, 0), pixel_step bytes apart horizontally, pitch[0] bytes between rows: RGB24 (step 3), RGBA (step 4,
 *                  base + 0 / 1 / 2), BGRA (step 4, base + 2 / 1 / 0), planar (step 1); converted with the BT.709 (default) or BT.601 matrix, limited (default) or full range,
 *                  in exact integer arithmetic (the stream signals no colour description: the application knows what it asked for).
 *   KS265_IN_RGB_F16 / _BF16 / _F32   the same layouts with float16, bfloat16 or float32 samples, [0, 1] the full 8-bit range (a model's or renderer's output as it lies):
 *                  plane, pixel_step and pitch[0] still in BYTES and multiples of the element size es (2, 2, 4), es <= pixel_step <= 64 (else QY_NOTSUPPORTED) - planar
 *                  (step es), HWC (3 es), four-element pixels (4 es).  One kernel reads the samples once; a float32 picture u8 / 255 codes as the picture u8 does, the
 *                  16-bit types within one code of it (tests/yuv_float_ref.py is the specification).
 *   KS265_IN_YUV(layout, sub, depth, msb)   what decoders, capture cards and renderers leave in device memory: YUV of 8 to 16 bits in 4:2:0, 4:2:2 or 4:4:4, reduced to the
 *                  encoder's 8-bit 4:2:0 by one kernel that reads the source once (tests/yuv_hibit_ref.py is the specification).  layout 0 planar (plane[0..2] = Y, U, V with
 *                  their own pitches), 1 semi-planar (plane[0] = Y, plane[1] = U,V interleaved, U first), 2 packed YUYV, 3 packed UYVY (plane[0] alone; 4:2:2 only); sub 0 =
 *                  4:2:0, 1 = 4:2:2, 2 = 4:4:4; depth 8 (bytes; msb 0) or 9 .. 16 (two-byte little-endian words: msb 1 = the sample is the TOP depth bits, as in P010 and
 *                  Y210, msb 0 = the LOW bits, as in yuv420p10le).  The names below cover the common ones.  Two-byte formats want even plane addresses and pitches.  Any other
 *                  combination is QY_NOTSUPPORTED.  Luma is rounded to 8 bits (ties up, clipped to 255); chroma is filtered at full depth - 4:2:2 by the vertical (1, 1)
 *                  filter, 4:4:4 by (1, 2, 1) x (1, 1) at HEVC's default siting, as the RGB path does - and rounded ONCE, together with the depth reduction.  No dither, and
 *                  no range or matrix conversion: the range that goes in comes out; pixel_step, matrix and full_range are ignored.
 * CONTRACT: the encoder reads the planes in the order of `stream` (a hipStream_t; NULL = the null stream): its work waits for everything the caller enqueued there before the
 * call, and everything the caller enqueues there after the call waits until the encoder has read the picture.  So the caller may overwrite the buffer with further work on that
 * same stream as soon as the call returns - no host synchronisation.  Work on OTHER streams must order itself against `stream`.  The call does not block on the GPU. */
#define KS265_IN_I420 0
#define KS265_IN_NV12 1
#define KS265_IN_RGB 2
#define KS265_IN_RGB_F16 16
#define KS265_IN_RGB_BF16 17
#define KS265_IN_RGB_F32 18
#define KS265_IN_YUV(layout, sub, depth, msb) (0x1000 | (layout) << 8 | (sub) << 6 | (msb) << 5 | (depth))
#define KS265_IN_I422 KS265_IN_YUV(0, 1, 8, 0)
#define KS265_IN_I444 KS265_IN_YUV(0, 2, 8, 0)
#define KS265_IN_NV16 KS265_IN_YUV(1, 1, 8, 0)
#define KS265_IN_NV24 KS265_IN_YUV(1, 2, 8, 0)
#define KS265_IN_YUYV KS265_IN_YUV(2, 1, 8, 0)
#define KS265_IN_UYVY KS265_IN_YUV(3, 1, 8, 0)
#define KS265_IN_I010 KS265_IN_YUV(0, 0, 10, 0)               /* planar, the low bits (yuv420p10le / yuv422p10le / yuv444p10le) */
#define KS265_IN_I210 KS265_IN_YUV(0, 1, 10, 0)
#define KS265_IN_I410 KS265_IN_YUV(0, 2, 10, 0)
#define KS265_IN_P010 KS265_IN_YUV(1, 0, 10, 1)               /* semi-planar, the top bits */
#define KS265_IN_P012 KS265_IN_YUV(1, 0, 12, 1)
#define KS265_IN_P016 KS265_IN_YUV(1, 0, 16, 1)
#define KS265_IN_P210 KS265_IN_YUV(1, 1, 10, 1)
#define KS265_IN_P410 KS265_IN_YUV(1, 2, 10, 1)
#define KS265_IN_Y210 KS265_IN_YUV(2, 1, 10, 1)               /* YUYV order, the top bits */
#define KS265_IN_Y216 KS265_IN_YUV(2, 1, 16, 1)
#define KS265_MATRIX_BT709 0
#define KS265_MATRIX_BT601 1
typedef struct ks265_dev_picture {
    int format;                                /* KS265_IN_I420 / _NV12 / _RGB / _RGB_F16 / _RGB_BF16 / _RGB_F32 / KS265_IN_YUV(...) (input only) */
    int device;                                /* HIP ordinal the planes live on */
    const void *plane[3]; int pitch[3];        /* bytes; RGB: channel pointers R, G, B and pitch[0] */
    int pixel_step;                            /* RGB only */
    int matrix, full_range;                    /* RGB only: KS265_MATRIX_BT709 (0, default) / _BT601; 0 = limited range */
    void *stream;                              /* hipStream_t the planes were produced on; NULL = the null stream */
    long long pts;
} ks265_dev_picture;
/* PICTURE SIZES.  QY265EncoderOpen takes any EVEN picWidth / picHeight up to 8192 (odd: QY_NOTSUPPORTED).  A size that is no multiple of 8 is coded at the next multiple of 8 (the
 * minimum CU size) and the SPS carries a conformance window - conf_win_right_offset = (coded width - picWidth) / 2, conf_win_bottom_offset likewise, left and top 0 - so a decoder
 * outputs picWidth x picHeight: what the reference's encoder does (854x480 -> 856x480 and 0, 1, 0, 0).  The device library pads (ks265_input_pad: last column and last row replicated),
 * crops and corrects the SSE; against a device library without those entries such a size is QY_NOTSUPPORTED with a log line.  On such a handle:
 *   - every picture is described at picWidth x picHeight: QY265YUV (QY265EncoderEncodeFrame, ks265_enc_acquire_input), ks265_dev_picture, the CLI's input file;
 *   - ks265_enc_encode_device_frame takes 8-bit KS265_IN_I420 and KS265_IN_NV12 only, planes at any pitch >= the row and any byte address; every other format, and
 *     ks265_enc_enable_device_scale / ks265_enc_encode_device_frame_scaled, return QY_NOTSUPPORTED - nothing is enqueued, the handle stays usable;
 *   - ks265_enc_get_device_recon fills picWidth x picHeight pictures in every format; ks265_enc_set_recon_file / -o writes picWidth x picHeight pictures;
 *   - -psnr / ks265_enc_get_quality: SSE and PSNR over the picWidth x picHeight window.  SSIM (-ssim) stays over the CODED picture, padding included; so does the decoded picture
 *     hash SEI, as H.265 D.3.19 defines it;
 *   - a `roi` map describes the source picture: ceil(picWidth / b) x ceil(picHeight / b) elements;
 *   - `analysis` arrays describe the CODED picture: ceil(picWidth / 8) x ceil(picHeight / 8) blocks (and ceil(. / 64) CTUs), block errors with the padding in them.
 * For sizes that are multiples of 8 nothing differs from before: no byte of a stream, no device-library call. */
int ks265_enc_enable_device_input(void *pEncoder);
int ks265_enc_encode_device_frame(void *pEncoder, QY265Nal **pNals, int *iNalCount, const ks265_dev_picture *pic, QY265Picture *pOutpic);
/* extension: device pictures of ANOTHER size, scaled to the encoder's on the GPU (one decoded or rendered picture into a ladder of handles).  The resampler is separable and
 * exact (tests/yuv_scale_ref.py is the specification): filter 0 = triangle (bilinear, widened when shrinking), 1 = Catmull-Rom (widened the same way); luma and
 * vertical chroma centre-sited, horizontal chroma cosited as HEVC's default siting; an RGB or KS265_IN_YUV source is converted at ITS size as above and the I420 picture is scaled.
 *   ks265_enc_enable_device_scale  after ks265_enc_enable_device_input, before the first picture: allocates per GOP lane one I420 picture of the largest source size (the RGB
 *       sources' way station) and nothing else.  QY_NOTSUPPORTED: device input off; after the first picture; a device library without the scaler (one log line "ks265enc: input
 *       scaling is unavailable: ..."); max_src_width no multiple of 8, max_src_height odd, either above 8192 or above 8 times the encoder's; an encoder whose width or height is
 *       no multiple of 8.
 *   ks265_enc_encode_device_frame_scaled  as ks265_enc_encode_device_frame - the same contract on `stream`, the same two events, no stream more - for a picture of
 *       src_width x src_height: width a multiple of 8, height even, within the maximum, each ratio to the encoder's size at most 8 either way (else QY_NOTSUPPORTED); planes are
 *       judged at the SOURCE's size (QY_POINTER).  A refused picture enqueues nothing and consumes no pending ROI map.  A source of the encoder's own size IS
 *       ks265_enc_encode_device_frame.  The scaled picture is what the encoder sees everywhere: lookahead, -aq, cuTree, lanes, hash, devrecon; a `roi` map refers to the
 *       encoder's size.  Each lane keeps the tables of its four most recent (source size, filter) pairs; a fifth replaces the least recently used: built on the calling thread, after a wait for
 *       the lane's upload stream - a source that cycles through more than four sizes pays that wait and the tables with every picture. */
int ks265_enc_enable_device_scale(void *pEncoder, int max_src_width, int max_src_height);
int ks265_enc_encode_device_frame_scaled(void *pEncoder, QY265Nal **pNals, int *iNalCount, const ks265_dev_picture *pic, int src_width, int src_height, int filter, QY265Picture *pOutpic);
/* extension: reconstructed pictures in device memory - the pictures a decoder of this stream will show, where they already lie.
 * "devrecon" (ks265_enc_set_default, 0 / 1, default 0; other values QY265_PARAM_BAD_VALUE; a process default read by the next QY265EncoderOpen, like "hash"; the environment's
 * KS265_DEVRECON=0|1 overrides it at open): every picture's output picture is packed as I420 into a slot of a pool in device memory (per lane the ring of pictures in flight,
 * + a GOP for a GOP lane; its bytes are logged at open), on whichever stream codes the picture - key pictures stay on their own stream, the stream is byte for byte the one without
 * the switch, and with the switch off not one call is added.  The scheduler waits for a free slot as it waits for ring space: it never drops a picture and never fails.  Refused at
 * open, with one `ks265enc: device reconstruction is unavailable: ...` line and the switch then off: a device library without ks265_output_convert, GOP lanes on several GPUs,
 * the KS265_GRAPH experiment.
 * When a call hands a picture's NAL units out, its reconstruction joins the handle's list, in the order of the call's NAL units (coding order).
 *   ks265_enc_device_recon_pending  how many reconstructions the last call handed out that have not been fetched yet;
 *   ks265_enc_get_device_recon      converts the OLDEST pending one into `dst` and fills info->poc (the display index in the stream, as pOutpic reports it, GOP lanes
 *                                   included), iSliceType and pts (info may be NULL).  Of `dst`: format, plane, pitch, pixel_step, matrix, full_range, device, stream; pts is
 *                                   ignored.  KS265_IN_I420 / _NV12 as for the input; KS265_IN_RGB with pixel_step 1 (planar), 3 (RGB24) or 4 - there the three channel
 *                                   pointers name three bytes of one four-byte pixel that begins at the lowest of them (RGBA, BGRA), and its fourth byte is written as 255.
 *                                   YCbCr -> RGB in exact integer arithmetic, chroma interpolated bilinearly at HEVC's default siting (tests/yuv_output_ref.py).  Nothing
 *                                   outside [row start, row start + row bytes) of a row is written: the padding behind a pitch stays.
 *                                   KS265_IN_RGB_F16 / _BF16 / _F32: the same picture as float samples - the float32 of byte / 255, correctly rounded (the 16-bit
 *                                   types rounded once more, to nearest even), so that sample x 255 is the uint8 reconstruction; pixel_step es (planar), 3 es or 4 es
 *                                   with es the element size, everything in bytes and a multiple of es; the fourth element of a four-element pixel is written as 1.0.
 *                                   QY_FAIL: nothing pending.  QY_POINTER: a plane whose whole extent does not lie inside one device allocation of the handle's GPU (host and
 *                                   managed memory, short buffers, pitches below the row) - the picture stays pending and nothing is enqueued.  QY_NOTSUPPORTED: the switch is
 *                                   off, dst->device is not the handle's GPU, or a format / pixel step outside the list.
 * CONTRACT: reconstructions live as long as the call's NAL array: the next QY265EncoderEncodeFrame / ks265_enc_encode_device_frame / QY265EncoderClose on the handle returns
 * every slot of the previous call to the pool, fetched or not.  The conversion is ordered as the input is, mirrored: it waits for the picture's pack and for everything the caller
 * enqueued on dst->stream before the call, and everything enqueued on dst->stream after the call waits for it (it runs as one kernel IN dst->stream, which must be a stream of
 * the handle's GPU and alive until the handle is closed) - the caller reads `dst` with further work on that stream at once.
 * No host synchronisation happens anywhere and ks265_enc_get_device_recon does not block on the GPU; a slot that is written again waits on its stream for the last conversion
 * that read it (an event per slot), so a conversion still in flight when its slot goes back to the pool is safe.
 * A handle whose size is no multiple of 8 (PICTURE SIZES above): TWO kernels run in dst->stream - the crop of the coded picture into a scratch picture of the lane (allocated at
 * QY265EncoderOpen with the pool: no allocation inside the call), then the conversion out of it.  Successive calls may name different streams: each call's crop waits in its
 * stream for the conversion that read the scratch picture last (one more event), so fetching on several streams is safe; those conversions then run one after another. */
int ks265_enc_device_recon_pending(void *pEncoder);
int ks265_enc_get_device_recon(void *pEncoder, const ks265_dev_picture *dst, QY265Picture *info);
/* extension: analysis out - what the encoder DECIDED about every picture, as arrays in device memory: the motion field and the reference each block points at, the CU tree,
 * intra / inter, the residual flags, the QP every CTU was finally coded with (after -aq, the cuTree and the caller's `roi` offsets) and the squared error every block was left with.
 * "analysis" (ks265_enc_set_default, 0 / 1, default 0; other values QY265_PARAM_BAD_VALUE; a process default read by the next QY265EncoderOpen, like "devrecon"; the environment's
 * KS265_ANALYSIS=0|1 overrides it at open): every picture's analysis is packed into a block in device memory by ONE kernel on whichever stream codes the picture, beside the
 * reconstruction's pack where "devrecon" is on too - the two switches share one pool (the slot numbers, the pool's size and the scheduler's wait for a free slot are devrecon's; a
 * slot owns a packed picture if devrecon is on and an analysis block if analysis is on; the added bytes are logged at open).  The stream is byte for byte the one without the
 * switch, and with the switch off not one call is added.  Refused at open, with one `ks265enc: analysis is unavailable: ...` line and the switch then off: a device library
 * without ks265_analysis_pack, GOP lanes on several GPUs, the KS265_GRAPH experiment.
 * With w8 x h8 = width / 8 x height / 8 blocks of 8 x 8 luma samples and cc x cr = ceil(width / 64) x ceil(height / 64) CTUs, the five fields (tests/analysis_ref.py is the
 * definition):
 *   mv   int16 [2][h8][w8][2]  list L's motion vector (x, y) in quarter samples; (0, 0) where the block does not use the list or is intra.  SIGN: a block at (x, y) predicts from
 *                              (x + mv.x / 4, y + mv.y / 4) of its reference picture - content that moves right between the reference and this picture has a NEGATIVE x
 *   ref  int8  [2][h8][w8]     display index of the reference picture the block uses in list L minus this picture's: negative = past; 0 = list unused or intra
 *   cu   uint8 [5][h8][w8]     plane 0: 0 intra, 1 list 0, 2 list 1, 3 bi-predicted; plane 1: log2 of the CU size (3 .. 6); plane 2: 0 = 2Nx2N, 1 / 2 = the two rectangular
 *                              shapes, 3 = four transform units; plane 3: coded block flags (bit 0 Y, 1 Cb, 2 Cr); plane 4: intra luma mode 0 .. 34, 255 for inter blocks
 *   qp   int8  [cr][cc]        the CTU's QP
 *   sse  int32 [3][h8][w8]     sum of (source - reconstruction)^2 over the block's 8 x 8 luma, 4 x 4 Cb and 4 x 4 Cr samples; a plane's sum is the picture's -psnr SSE
 * (Skip and merge flags are decided by the slice writer on the host and are not part of the analysis.)
 * Each field of ks265_dev_analysis: data (NULL = not wanted), pitch = bytes between rows, plane = bytes between planes (ignored for qp); rows are dense.
 * When a call hands a picture's NAL units out, its analysis joins the handle's list, in the order of the call's NAL units (coding order).
 *   ks265_enc_device_analysis_pending  how many analyses the last call handed out that have not been fetched yet;
 *   ks265_enc_get_device_analysis      copies the wanted fields of the OLDEST pending one into `dst` and fills info->poc (the display index in the stream, as pOutpic reports
 *                                      it, GOP lanes included), iSliceType and pts (info may be NULL).  Nothing outside [row start, row start + row bytes) of a row is
 *                                      written.  QY_FAIL: nothing pending.  QY_POINTER: a wanted field whose whole extent does not lie inside one device allocation of the
 *                                      handle's GPU, whose pitch is below its row, whose pitch, plane step or address is no multiple of its element size, or no field wanted
 *                                      at all - the picture stays pending and nothing is enqueued.  QY_NOTSUPPORTED: the switch is off or dst->device is not the handle's GPU.
 * CONTRACT: that of ks265_enc_get_device_recon.  Analyses live as long as the call's NAL array: the next encode, flush or close call on the handle takes every slot back,
 * fetched or not.  The copy waits for the picture's packs and for everything the caller enqueued on dst->stream before the call, runs as one kernel IN dst->stream, and
 * everything enqueued there after the call waits for it.  The call never blocks on the GPU; a block that is written again waits on its stream for the last copy that read it.
 * Analyses and reconstructions of the same call are fetched independently of each other, in any interleaving. */
typedef struct ks265_dev_analysis {
    int device;                                /* HIP ordinal the arrays live on */
    void *stream;                              /* hipStream_t the arrays are used on; NULL = the null stream */
    struct { void *data; int pitch; long long plane; } mv, ref, cu, qp, sse;
} ks265_dev_analysis;
int ks265_enc_device_analysis_pending(void *pEncoder);
int ks265_enc_get_device_analysis(void *pEncoder, const ks265_dev_analysis *dst, QY265Picture *info);
/* extension: ROI - a map of quantiser offsets per picture, from host or device memory ("spend bits here, save them there"; x265's quantOffsets, a QP-delta map).
 * "roi" (ks265_enc_set_default, 0 / 1, default 0; other values QY265_PARAM_BAD_VALUE; a process default read by the next QY265EncoderOpen, like "hash"; the environment's
 * KS265_ROI=0|1 overrides it at open; `ks265enc -roi x:y:w:h:dqp` implies it): the stream carries one QP per CTU (cu_qp_delta_enabled_flag = 1 in the PPS, as with -aq and the
 * cuTree - and, like them, no KS265_GRAPH experiment and no anchor lane).  With the switch off not one call is added and every stream keeps its bytes.  Refused at open, with one
 * `ks265enc: ROI maps are unavailable: ...` line and the switch then off: a device library without ks265_roi_reduce / ks265_roi_ctu_map, GOP lanes on several GPUs.
 * A map is a 2-D array of QP offsets, positive = coarser: KS265_ROI_INT8 or KS265_ROI_FLOAT32 elements, one per b x b luma block, b = 1 << log2_block (0 .. 6: from a per-pixel
 * mask to one value per CTU), ceil(width / b) x ceil(height / b) elements, `pitch` bytes between rows (at least the row, a multiple of the element size).  The CTU's offset is
 * the mean of its elements (each clipped to [-51, 51]; a non-finite float counts 0), exact in 1/256 QP (tests/roi_map_ref.py is the definition); it is added to
 * the mean of the CTU's -aq or cuTree offsets before that sum is rounded and clipped to +-12 around the picture's QP.  The lookahead and the cuTree do NOT see the caller's
 * offsets: slice types, the tree's propagation and the rate controllers' complexity figures are those of the stream without maps.
 *   ks265_enc_set_next_roi  describes the map of the NEXT picture handed in, by either encode entry point (a flush call does not consume it); NULL withdraws a pending one.  A
 *                           picture handed in with nothing pending is coded without caller offsets.  Validated at once; on any refusal nothing is pending:
 *                           QY_NOTSUPPORTED  the switch is off, roi->device is neither -1 nor the handle's GPU, or a type / log2_block / pitch outside the list;
 *                           QY_POINTER       NULL data, or a device map whose extent [data, data + pitch (rows - 1) + row bytes) does not lie inside one device allocation.
 * CONTRACT: the map is read inside the next encode call.  A host map (device = -1) must stay valid until that call returns.  A device map is read in the order of roi->stream,
 * as ks265_dev_picture's planes are: the encoder's read waits for everything enqueued there before the encode call, and everything enqueued there after it waits for the read -
 * the caller may overwrite the map on that stream as soon as the encode call returns. */
#define KS265_ROI_INT8 0
#define KS265_ROI_FLOAT32 1
typedef struct ks265_roi {
    int type;                                  /* KS265_ROI_INT8 / _FLOAT32 */
    int log2_block;                            /* 0 .. 6 */
    int device;                                /* HIP ordinal, -1 = host memory */
    const void *data; int pitch; void *stream;
} ks265_roi;
int ks265_enc_set_next_roi(void *pEncoder, const ks265_roi *roi);   /* NULL withdraws */
/* extension: overlays - a station logo or watermark, burnt-in captions, a timestamp, a picture in picture - blended onto every picture on the GPU as the LAST step on its way
 * in, in the encoder's own matrix-free terms: the overlay is RGB plus alpha with ITS matrix and range, the picture is the YCbCr the encoder codes (DESIGN.md 4u;
 * tests/overlay_ref.py is the specification of every byte).  Eight slots, 0 .. 7, blended in ascending slot number where they overlap.  With no overlay set there is no call,
 * no allocation, no log line and no changed stream byte.
 *   rgb            the samples, as ks265_enc_encode_device_frame describes an RGB picture: format KS265_IN_RGB / _RGB_F16 / _RGB_BF16 / _RGB_F32, plane[0..2] = the R, G, B
 *                  sample of pixel (0, 0), pitch[0], pixel_step, matrix, full_range; device = the handle's GPU (read on `stream`) or -1 = host memory; pts is ignored
 *   width, height  even, 2 .. 8192
 *   alpha          the alpha sample of pixel (0, 0): the same element type, pixel_step and pitch as the colours (RGBA: rgb.plane[0] + 3 elements' bytes); NULL = opaque
 *   x, y           the top-left corner in the ENCODER's picture (behind the scaler; picWidth x picHeight): even, any sign, -16384 .. 16384; the part outside is clipped.  On a
 *                  handle whose size is no multiple of 8 the rectangle is clipped to picWidth x picHeight: the padding keeps the bytes it had
 *   opacity        0 .. 256 on top of the alpha samples (256 = as they are)
 *   flags          KS265_OV_FORCED_ONLY: drawn only on pictures whose QY265EncoderEncodeFrame call passed bForceLogo != 0 - the SDK's slot for "this picture carries the
 *                  logo" - and never for ks265_enc_encode_device_frame[_scaled].  With no such overlay set bForceLogo stays without effect
 * Float samples count as the 8-bit code nearest to them ([0, 1] the full range, NaN = 0); an opaque overlay is byte for byte what the encoder's own RGB conversion makes of it;
 * chroma is filtered from premultiplied samples, so the colour of transparent pixels never bleeds in.
 *   ks265_enc_set_overlay  sets, replaces or (ov = NULL) clears a slot.  In force from the NEXT picture handed in, by either entry point, until replaced or cleared; pictures
 *       handed in before keep what they had.  The set travels with the picture: one GOP lane and several give the same bytes.  Validated at once; on any refusal the slot keeps
 *       what it had:  QY_POINTER - a NULL handle or channel, or a device overlay whose extent (every channel's, alpha's included: [p, p + pitch (height - 1) + row bytes)) does
 *       not lie inside one device allocation of the handle's GPU;  QY_NOTSUPPORTED - slot, size, parity, position, opacity, flags, format, pixel step or matrix outside the
 *       list, rgb.device neither -1 nor the handle's GPU, GOP lanes on several GPUs, the KS265_GRAPH experiment, a device library without ks265_input_overlay (one log line
 *       `ks265enc: overlays are unavailable: ...`);  QY_OUTOFMEMORY.  With overlays in force every input slot needs a twin in device memory, as the vpp_* filters arrange at
 *       open: a handle that has none yet (no lookahead, no filter, no device input) gets them inside the first ks265_enc_set_overlay call that sets an overlay, which therefore
 *       wants no picture in flight - before the first picture, on a zero-latency handle, or after a flush; else QY_NOTSUPPORTED with a log line.
 * CONTRACT: a DEVICE overlay is read in place inside every encode call, in the order of ov->rgb.stream, as ks265_dev_picture's planes are: the caller may rewrite it with work
 * on that stream as soon as an encode call returns - that is how captions animate, with no host synchronisation - and it must stay allocated until the slot is cleared or
 * replaced and the pictures handed in before that have been read (a flush, or a synchronisation of that stream after the next encode call).  A HOST overlay (device = -1) is
 * copied inside the set call into device memory the handle owns - the buffer is the caller's again on return - shared read-only by the lanes and freed at clear, replace and
 * close; its channels are those of ONE buffer (everything between the lowest and the highest of them is copied: at most four planes apart, else QY_NOTSUPPORTED).
 * What sees the overlay: everything behind the input - lookahead, -aq, cuTree, -psnr / -ssim (against the overlaid picture), `analysis`, `devrecon`, the hash.  What does not:
 * the vpp_* filters, which run in front of it, and the denoiser's history - a logo is never smeared into later pictures. */
typedef struct ks265_overlay {
    ks265_dev_picture rgb;                     /* device = -1: host memory; pts ignored */
    int width, height;
    const void *alpha;                         /* NULL = opaque */
    int x, y, opacity /* 0 .. 256 */, flags;
} ks265_overlay;
#define KS265_OV_FORCED_ONLY 1
#define KS265_OV_SLOTS 8
int ks265_enc_set_overlay(void *pEncoder, int slot /* 0 .. 7 */, const ks265_overlay *ov /* NULL clears the slot */);
/* extension: tone mapping on the way in - HDR10 device pictures (SMPTE ST 2084 "PQ", BT.2020 primaries and matrix; P010, P012, P016, yuv420p10le ...) become the 8-bit SDR
 * picture the encoder codes, BT.709 in limited range, inside the ONE kernel that reads the source (tests/tonemap_ref.py is the specification of every byte).
 * Without it such a picture is only rounded to 8 bits, PQ codes and BT.2020 colours as they are.  Call after ks265_enc_enable_device_input and before the first picture.
 *   transfer       16 = PQ (H.273's code).  Anything else is QY_NOTSUPPORTED: HLG is not built yet
 *   curve          0 bt2390 (BT.2390's EETF in PQ space: identity below the knee, a Hermite roll-off to the peak), 1 reinhard, 2 clip.  The gain is taken on the largest
 *                  of R, G and B, so hue is preserved
 *   full_range     of the SOURCE (the result is always limited range)
 *   peak_nits      the light that maps to SDR white's top; 0 = 1000; 100 .. 10000.  What the source holds above it is clipped to it
 *   white_nits     the light that diffuse SDR white (1.0) stands for; 0 = 203 (BT.2408); 80 .. 1000 and at most the peak
 * From then on ks265_enc_encode_device_frame[_scaled] sends every picture of format KS265_IN_YUV(0 or 1, 0, 10 .. 16, msb) - 4:2:0, planar or semi-planar - through the
 * tone mapper where it would be converted; the scaled entry maps at the source's size and scales the SDR picture.  A YUV picture of more than 8 bits outside that list
 * (9 bits, 4:2:2, 4:4:4, packed) is QY_NOTSUPPORTED - never passed through unmapped - and leaves the handle as it was.  8-bit YUV, RGB and host pictures go in as before.
 * Everything behind the input sees the SDR picture: the vpp_* filters, overlays, lookahead, -psnr / -ssim, `analysis`, `devrecon`.  The filter has no state: any number of GOP
 * lanes gives the one-lane stream.  The stream's VUI stays the caller's business, as for RGB input.  A handle that never calls this makes not one more call.
 * QY_NOTSUPPORTED: a call in any other order or a second one, a field out of range, a handle whose size is no multiple of 8 (device input takes 8-bit I420 / NV12 only there),
 * a device library without the entries (one log line `ks265enc: tone mapping is unavailable: ...`).  The command line has no switch for it: it reads 8-bit host files only. */
typedef struct ks265_tonemap { int transfer;      /* 16 = PQ (H.273's code); anything else QY_NOTSUPPORTED - HLG is left for later */
                               int curve;         /* 0 bt2390, 1 reinhard, 2 clip */
                               int full_range;    /* of the SOURCE */
                               double peak_nits;  /* 0 = 1000; 100 .. 10000 */
                               double white_nits; /* 0 = 203 (BT.2408); 80 .. 1000, <= peak */ } ks265_tonemap;
int ks265_enc_enable_tonemap(void *pEncoder, const ks265_tonemap *tm);
/* extension: write the reconstruction (I420, display order) to `path` - the reference CLI's `-o`; call between Open and the first picture */
int ks265_enc_set_recon_file(void *pEncoder, const char *path);

#ifdef __cplusplus
}
#endif
#endif
