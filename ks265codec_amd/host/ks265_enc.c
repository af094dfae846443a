/* ks265_enc.c — the encoder behind the SDK's library API (include/ks265_enc.h; SURVEY.md §8(b) "B2", caller sequence §3.4):
 * QY265ConfigDefault* -> QY265EncoderOpen -> QY265EncoderEncodeFrame ... -> flush -> QY265EncoderClose.
 *
 * Plain C host over two C ABIs: libks265hip.so (the pixel path on the MI355X, include/ks265_hip.h) and the bitstream writer
 * (ks265_stream.c).  What the reference's host does per frame (CHevcEncode::encodeFrame enc@0x4b9930, §3.2) maps to:
 *   input picture -> pinned host copy -> H2D (copy-in stream) -> ks265_encode_picture[_b/_mref] (all pixel stages on the compute stream)
 *   -> records to a staging set (D2D) -> D2H of the CU map / levels / SAO records (copy-out stream, pinned) -> event; the three streams hand
 *      over by events, so the copies of neighbouring pictures run under the kernels of the current one
 *   -> a host thread waits for the event and writes the slice NAL (CABAC), one picture per thread, pictures of a GOP in parallel
 *   -> NAL units are handed out in coding order (the SDK's asynchronous contract: output lags input).
 * GOP structures: IPPP (optionally several list-0 pictures), anchor + n non-reference B, hierarchical-B mini-GOPs of 8 (the SDK's
 * default at default latency); every key picture is an IDR (closed GOPs: what GOP-sharding over GPUs needs).
 */
#define _GNU_SOURCE
#include "ks265_enc.h"
#include "ks265_stream.h"
#include "ks265_gop.h"
#include "ks265_recon.h"
#include "ks265_roi.h"
#include "ks265_scale.h"
#include "ks265_tonemap.h"
#include <dirent.h>
#include <fcntl.h>
#include <math.h>
#include <pthread.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <unistd.h>
/* device input (ks265_enc_encode_device_frame) reaches these entry points of libks265hip.so as weak symbols: a device library without them - the CPU tests' stand-in - leaves
 * them NULL, and the device input is QY_NOTSUPPORTED */
#pragma weak ks265_input_validate
#pragma weak ks265_input_convert
#pragma weak ks265_wait_external
#pragma weak ks265_external_wait_event
/* -ssim (calcSsim) reaches the fused SSIM + SSE pass the same way: on a device library without it the encoder works as before, logs once that SSIM is unavailable
 * and prints no ` ssim:` line */
#pragma weak ks265_ssim_picture
#pragma weak ks265_ssim_picture_on
/* `hash` (decoded picture hash SEI messages) reaches the hash pass the same way: on a device library without it the encoder logs once that the picture hash is unavailable
 * and writes the stream it writes without the switch */
#pragma weak ks265_picture_hash
#pragma weak ks265_picture_hash_on
/* `devrecon` (reconstructed pictures handed out in device memory) reaches the way back the same way: on a device library without it the encoder logs once that device
 * reconstruction is unavailable and ks265_enc_get_device_recon is QY_NOTSUPPORTED */
#pragma weak ks265_output_validate
#pragma weak ks265_output_convert
#pragma weak ks265_set_stream
/* `roi` (the caller's quantiser offset maps) reaches the map's reduction and the combination with the -aq / cuTree offsets the same way: on a device library without them the
 * encoder logs once that ROI maps are unavailable and ks265_enc_set_next_roi is QY_NOTSUPPORTED */
#pragma weak ks265_roi_validate
#pragma weak ks265_roi_reduce
#pragma weak ks265_roi_ctu_map
/* `gpb` switches the skip pass off for its anchors the same way: a device library without the setter - the stand-in has no skip pass - is not asked */
#pragma weak ks265_frame_set_picture_skip
/* device input of another size (ks265_enc_enable_device_scale): the scaler's entries; without them the switch is refused with one log line */
#pragma weak ks265_scale_plan_create
#pragma weak ks265_scale_plan_destroy
#pragma weak ks265_input_scale
/* `analysis` (what the encoder decided about a picture, fetched as arrays in device memory) reaches the pack and the export the same way: on a device library without them the
 * encoder logs once that the analysis is unavailable and ks265_enc_get_device_analysis is QY_NOTSUPPORTED */
#pragma weak ks265_analysis_bytes
#pragma weak ks265_analysis_pack
#pragma weak ks265_analysis_validate
#pragma weak ks265_analysis_export
/* picture sizes that are no multiple of 8 reach the padding, the crop and the window's SSE the same way: on a device library without them such a size is
 * QY_NOTSUPPORTED at QY265EncoderOpen, with one log line, as every such size was before */
#pragma weak ks265_input_pad_validate
#pragma weak ks265_input_pad
#pragma weak ks265_output_crop
#pragma weak ks265_sse_window
/* `vpp_denoise` / `vpp_recur_filter` (ks265_enc.h): the temporal filter behind whatever made the input slot's twin.  A handle that asks for it on a device library without the
 * two entries is refused at open (QY_NOTSUPPORTED, one log line) */
#pragma weak ks265_input_denoise_validate
#pragma weak ks265_input_denoise
/* `vpp_edge` / `vpp_color` (ks265_enc.h): the stateless enhancement behind the denoiser, the last step in front of the encoder.  Refused at open in the same way */
#pragma weak ks265_input_enhance_validate
#pragma weak ks265_input_enhance
/* `vpp_hdr` (ks265_enc.h): the local-contrast filter between the denoiser and the enhancement.  Refused at open in the same way */
#pragma weak ks265_input_hdr_validate
#pragma weak ks265_input_hdr_work_bytes
#pragma weak ks265_input_hdr
/* overlays (ks265_enc_set_overlay, ks265_enc.h): the blend behind everything else on the way in.  Against a device library without the two entries the setter is
 * QY_NOTSUPPORTED with one log line */
#pragma weak ks265_input_overlay_validate
#pragma weak ks265_input_overlay
/* tone mapping on the way in (ks265_enc_enable_tonemap) reaches its plan and its kernel the same way: on a device library without them the encoder logs once that tone mapping
 * is unavailable and the call is QY_NOTSUPPORTED */
#pragma weak ks265_tonemap_plan_create
#pragma weak ks265_tonemap_plan_destroy
#pragma weak ks265_input_tonemap_validate
#pragma weak ks265_input_tonemap

const char strLibQy265Version[] = "ks265enc 0.2 (MI355X pixel path + host CABAC; API of libqycodec V2.6.1.3)";

static QYLogPrintf g_log_cb;
static unsigned long g_q_seq;                             /* pictures accounted by any lane of any handle: which lane's last picture is THE last one (ks265_enc_get_quality) */
void QY265SetLogPrintf(QYLogPrintf cb) { g_log_cb = cb; }
static void logf_(int level, int min_level, const char *fmt, ...)
{
    if (level < min_level) return;
    char buf[512];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    if (g_log_cb) g_log_cb(buf); else { fputs(buf, stdout); fflush(stdout); }
}

/* ---- MD5 (RFC 1321) of the reconstructed planes: the reference CLI's `-md5 1` lines `POC n MD5 y,u,v` (README.md:61-66 conventions) */
static void md5_block(uint32_t st[4], const uint8_t *p)
{
    static const uint8_t sh[64] = {7, 12, 17, 22, 7, 12, 17, 22, 7, 12, 17, 22, 7, 12, 17, 22, 5, 9, 14, 20, 5, 9, 14, 20, 5, 9, 14, 20, 5, 9, 14, 20,
                                   4, 11, 16, 23, 4, 11, 16, 23, 4, 11, 16, 23, 4, 11, 16, 23, 6, 10, 15, 21, 6, 10, 15, 21, 6, 10, 15, 21, 6, 10, 15, 21};
    static const uint32_t K[64] = {   /* floor(2^32 |sin(i + 1)|): a constant table (it used to be filled lazily by whichever writer thread came first) */
        0xd76aa478u, 0xe8c7b756u, 0x242070dbu, 0xc1bdceeeu, 0xf57c0fafu, 0x4787c62au, 0xa8304613u, 0xfd469501u, 0x698098d8u, 0x8b44f7afu, 0xffff5bb1u, 0x895cd7beu, 0x6b901122u, 0xfd987193u, 0xa679438eu, 0x49b40821u, 0xf61e2562u, 0xc040b340u, 0x265e5a51u, 0xe9b6c7aau, 0xd62f105du, 0x02441453u, 0xd8a1e681u, 0xe7d3fbc8u, 0x21e1cde6u, 0xc33707d6u, 0xf4d50d87u, 0x455a14edu, 0xa9e3e905u, 0xfcefa3f8u, 0x676f02d9u, 0x8d2a4c8au, 0xfffa3942u, 0x8771f681u, 0x6d9d6122u, 0xfde5380cu, 0xa4beea44u, 0x4bdecfa9u, 0xf6bb4b60u, 0xbebfbc70u, 0x289b7ec6u, 0xeaa127fau, 0xd4ef3085u, 0x04881d05u, 0xd9d4d039u, 0xe6db99e5u, 0x1fa27cf8u, 0xc4ac5665u, 0xf4292244u, 0x432aff97u, 0xab9423a7u, 0xfc93a039u, 0x655b59c3u, 0x8f0ccc92u, 0xffeff47du, 0x85845dd1u, 0x6fa87e4fu, 0xfe2ce6e0u, 0xa3014314u, 0x4e0811a1u, 0xf7537e82u, 0xbd3af235u, 0x2ad7d2bbu, 0xeb86d391u};
    uint32_t w[16], a = st[0], b = st[1], c = st[2], d = st[3];
    for (int i = 0; i < 16; ++i) w[i] = (uint32_t)p[4 * i] | (uint32_t)p[4 * i + 1] << 8 | (uint32_t)p[4 * i + 2] << 16 | (uint32_t)p[4 * i + 3] << 24;
    for (int i = 0; i < 64; ++i) {
        uint32_t f; int g;
        if (i < 16) { f = (b & c) | (~b & d); g = i; }
        else if (i < 32) { f = (d & b) | (~d & c); g = (5 * i + 1) & 15; }
        else if (i < 48) { f = b ^ c ^ d; g = (3 * i + 5) & 15; }
        else { f = c ^ (b | ~d); g = (7 * i) & 15; }
        const uint32_t t = d; d = c; c = b;
        const uint32_t x = a + f + K[i] + w[g];
        b = b + ((x << sh[i]) | (x >> (32 - sh[i]))); a = t;
    }
    st[0] += a; st[1] += b; st[2] += c; st[3] += d;
}
static void md5_hex(const uint8_t *data, size_t n, char out[33])
{
    uint32_t st[4] = {0x67452301u, 0xefcdab89u, 0x98badcfeu, 0x10325476u};
    size_t i = 0;
    for (; i + 64 <= n; i += 64) md5_block(st, data + i);
    uint8_t tail[128]; size_t r = n - i;
    memcpy(tail, data + i, r); tail[r++] = 0x80;
    const size_t padded = r <= 56 ? 64 : 128;
    memset(tail + r, 0, padded - r);
    const uint64_t bits = (uint64_t)n * 8;
    for (int k = 0; k < 8; ++k) tail[padded - 8 + k] = (uint8_t)(bits >> (8 * k));
    md5_block(st, tail); if (padded == 128) md5_block(st, tail + 64);
    for (int k = 0; k < 16; ++k) snprintf(out + 2 * k, 3, "%02x", (unsigned)((st[k >> 2] >> (8 * (k & 3))) & 255u));
}

/* CLI-level switches of `appencoder` that the SDK's QY265EncConfig has no field for (-df, -fixqp, -md5): process-wide defaults a front end
 * sets before QY265EncoderOpen (ks265_enc_set_default) */
static struct { int df, fixqp, md5, scenecut, cutree, gpb, hash, devrecon, roi, analysis; } g_cli = {1, 0, 0, 0, 1, 0, 0, 0, 0, 0};
int ks265_enc_set_default(const char *name, int value)
{
    if (!name) return QY_POINTER;
    if (!strcmp(name, "df")) { if (value < 0 || value > 1) return QY265_PARAM_BAD_VALUE; g_cli.df = value; return QY_OK; }
    if (!strcmp(name, "fixqp")) { if (value < 0 || value > 1) return QY265_PARAM_BAD_VALUE; g_cli.fixqp = value; return QY_OK; }
    if (!strcmp(name, "md5")) { if (value < 0 || value > 1) return QY265_PARAM_BAD_VALUE; g_cli.md5 = value; return QY_OK; }
    if (!strcmp(name, "scenecut")) { if (value < 0 || value > 100) return QY265_PARAM_BAD_VALUE; g_cli.scenecut = value; return QY_OK; }   /* the reference's hidden -scenecut N */
    if (!strcmp(name, "cutree")) { if (value < 0 || value > 1) return QY265_PARAM_BAD_VALUE; g_cli.cutree = value; return QY_OK; }        /* the reference's hidden -cutree N (on by default, as there) */
    if (!strcmp(name, "gpb")) { if (value < 0 || value > 1) return QY265_PARAM_BAD_VALUE; g_cli.gpb = value; return QY_OK; }                /* anchors as B slices over past anchors (ks265_enc.h) */
    /* decoded picture hash SEI messages, x265's numbering: 0 off, 2 CRC, 3 checksum; 1 (MD5) is refused - MD5 is sequential per plane, it stays with -md5's log lines (ks265_enc.h) */
    if (!strcmp(name, "hash")) { if (value != 0 && value != 2 && value != 3) return QY265_PARAM_BAD_VALUE; g_cli.hash = value; return QY_OK; }
    if (!strcmp(name, "devrecon")) { if (value < 0 || value > 1) return QY265_PARAM_BAD_VALUE; g_cli.devrecon = value; return QY_OK; }   /* reconstructions stay fetchable in device memory (ks265_enc.h) */
    if (!strcmp(name, "roi")) { if (value < 0 || value > 1) return QY265_PARAM_BAD_VALUE; g_cli.roi = value; return QY_OK; }             /* quantiser offset maps of the caller's (ks265_enc.h) */
    if (!strcmp(name, "analysis")) { if (value < 0 || value > 1) return QY265_PARAM_BAD_VALUE; g_cli.analysis = value; return QY_OK; }   /* motion, modes, QP and block error stay fetchable in device memory (ks265_enc.h) */
    return QY265_PARAM_BAD_NAME;
}

/* motion lambda in Q4 per QP: round(16 * sqrt(0.57 * 2^((qp - 12) / 3))) - the host-side float setup of the pixel path, as a table so that
 * every host (this one, the Python test mirror ks265codec_amd/synth.py) uses identical integers */
static const int kLambdaQ4[52] = {3, 3, 4, 4, 5, 5, 6, 7, 8, 9, 10, 11, 12, 14, 15, 17, 19, 22, 24, 27, 30, 34, 38, 43, 48, 54, 61, 68, 77, 86, 97, 108, 122, 137, 153, 172,
                                  193, 217, 244, 273, 307, 344, 387, 434, 487, 547, 614, 689, 773, 868, 974, 1093};

/* P / B pictures: lambda_mode carries HM's factor for pictures that are not key pictures, clip(2, 4, (qp - 12) / 6) - round(16 * sqrt(0.57 * f * 2^((qp - 12) / 3))).
 * The reference's own integer motion lambda (read from its mvd cost tables, tests/test_me_search.py: 8 at qp 27, 9 at 28, 16 at 33, 18 at 34) is within 10 percent of it.
 * It prices vectors, CU splits, merge, SAO and the coefficient-group pruning (ks265_frame_cfg.rdo) of those pictures; measured effect: DESIGN.md */
static const int kLambdaInterQ4[52] = {4, 5, 5, 6, 7, 8, 9, 10, 11, 12, 14, 15, 17, 19, 22, 24, 27, 30, 34, 38, 43, 48, 54, 61, 68, 80, 93, 108, 125, 145, 167, 193, 222, 256, 294, 337, 387, 434, 487, 547, 614, 689, 773, 868, 974, 1093, 1227, 1378, 1546, 1736, 1948, 2187};

/* ------------------------------------------------------------------ configuration (QY265ConfigDefault enc@0x4b7020 lineage: fillCfgs<Preset>) */
static const char *const kPresetNames[] = {"ultrafast", "superfast", "veryfast", "fast", "medium", "slow", "slower", "veryslow", "placebo", 0};
static const char *const kTuneNames[] = {"default", "selfshow", "game", "movie", "screen", 0};
static const char *const kLatencyNames[] = {"zerolatency", "lowdelay", "livestreaming", "default", 0};
/* tools per preset as the reference resolves them (measured from the CLI's config echo) */
static const struct { int me, subme, ref, ref0, part, tuinter, rdoq, sao; } kPresetTools[9] = {
    {1, 1, 1, 2, 0, 0, 0, 1}, {1, 1, 1, 3, 0, 0, 0, 1}, {1, 1, 1, 3, 0, 0, 0, 3}, {1, 1, 1, 3, 0, 0, 1, 3}, {1, 1, 1, 3, 0, 0, 1, 4},
    {2, 1, 1, 3, 0, 0, 1, 4}, {2, 1, 2, 4, 1, 0, 1, 4}, {2, 2, 4, 4, 1, 1, 1, 4}, {2, 2, 5, 5, 1, 2, 1, 4}};

/* what the reference's presets put into the configuration words its sub-pel refinement reads (cfg+0x464 = tME+0x3c0, tME+0x3c4, cfg+0x498, cfg+0x49c, cfg+0x580,
 * tME+0x64): measured inside real appencoder runs (oracle/ref_probe/subme_shim.c).  The public QY265EncConfig has no fields for them: they follow the preset.
 * ks265codec_amd/synth.py SUBME_PRESET holds the same table for the tests. */
static const struct { int thr, flat, cap, cap_step, diag_fast, satd; } kPresetSubme[9] = {
    {80, 40, 6, 6, 1, 0}, {76, 36, 6, 6, 1, 0}, {68, 16, 12, 6, 0, 0}, {56, 14, 0, 0, 0, 0}, {40, 10, 0, 0, 0, 0},
    {24, 8, 0, 0, 0, 0}, {24, 8, 0, 0, 0, 0}, {0, 8, 0, 0, 0, 1}, {0, 8, 0, 0, 0, 1}};

int QY265ConfigDefault(QY265EncConfig *c, QY265Preset preset, QY265Tune tune, QY265Latency latency)
{
    if (!c) return QY_POINTER;
    if ((int)preset < 0 || (int)preset > 8 || (int)tune < 0 || (int)tune > 4 || (int)latency < 0 || (int)latency > 3) return QY_NOTSUPPORTED;
    memset(c, 0, sizeof *c);
    c->tune = tune; c->preset = preset; c->latency = latency;
    c->profileId = 1; c->bHeaderBeforeKeyframe = 1; c->frameRate = 25.0;
    c->bframes = -1; c->rc = 2; c->bitrateInkbps = 1000; c->qp = 26; c->crf = 24; c->visual_quality = 95; c->iIntraPeriod = 256;
    c->qpmin = 0; c->qpmax = 51; c->enWavefront = 1; c->enFrameParallel = 1; c->threads = 0;
    c->logLevel = 0; c->lookahead = -1; c->fRateTolerance = 2.0;
    c->rdoq = kPresetTools[preset].rdoq; c->me = kPresetTools[preset].me; c->part = kPresetTools[preset].part; c->do64 = 1;
    c->tuInter = kPresetTools[preset].tuinter; c->tuIntra = kPresetTools[preset].tuinter; c->smooth = 1; c->transskip = 0;
    c->subme = kPresetTools[preset].subme; c->satdInter = preset >= QY265PRESET_SLOW; c->satdIntra = preset >= QY265PRESET_SLOW;
    c->searchrange = 64; c->refnum = kPresetTools[preset].ref; c->ref0 = kPresetTools[preset].ref0; c->sao = kPresetTools[preset].sao;
    c->iAqMode = 0; c->fAqStrength = 1.0; c->rasl = 1;
    return QY_OK;
}
static int find_name(const char *const *names, const char *s)
{
    if (!s) return -2;
    for (int i = 0; names[i]; ++i) if (!strcmp(names[i], s)) return i;
    return -1;
}
int QY265ConfigDefaultPreset(QY265EncConfig *c, char *preset, char *tune, char *latency)
{
    int p = find_name(kPresetNames, preset), t = find_name(kTuneNames, tune), l = find_name(kLatencyNames, latency);
    if (p == -2) p = QY265PRESET_MEDIUM;
    if (t == -2) t = QY265TUNE_DEFAULT;
    if (l == -2) l = QY265LATENCY_DEFAULT;
    if (p < 0 || t < 0 || l < 0) return QY_NOTSUPPORTED;
    return QY265ConfigDefault(c, (QY265Preset)p, (QY265Tune)t, (QY265Latency)l);
}
int QY265ConfigParse(QY265EncConfig *c, const char *name, const char *value)
{
    if (!c || !name || !value) return QY265_PARAM_BAD_NAME;
    char *end = NULL;
    const double dv = strtod(value, &end);
    const int num_ok = end && end != value && *end == 0, iv = (int)dv;
#define INTP(NAME, FIELD, LO, HI) if (!strcmp(name, NAME)) { if (!num_ok || iv < (LO) || iv > (HI)) return QY265_PARAM_BAD_VALUE; c->FIELD = iv; return 0; }
    INTP("wdt", picWidth, 2, 8192) INTP("hgt", picHeight, 2, 8192) INTP("bframes", bframes, -1, 15) INTP("rc", rc, 0, 5) INTP("br", bitrateInkbps, 1, 1000000)
    INTP("qp", qp, 0, 51) INTP("crf", crf, 0, 51) INTP("iper", iIntraPeriod, -1, 100000) INTP("qpmin", qpmin, 0, 51) INTP("qpmax", qpmax, 0, 51)
    INTP("threads", threads, 0, 1024) INTP("psnr", calcPsnr, 0, 2) INTP("ssim", calcSsim, 0, 2) INTP("log", logLevel, -1, 3) INTP("lookahead", lookahead, -1, 250)
    /* rdoq (qy265enc.h:129): every preset from `fast` up resolves to 1, which this build runs as its own seam (dead zone, coefficient-group pruning, sign-data hiding); asked for BY
     * NAME, rdoq 1 is stored as 2 = the reference's rdoQuant between the two halves of the reconstruction (ks265_frame_set_rdoq), so that the presets' streams stay what they are */
    if (!strcmp(name, "rdoq")) { if (!num_ok || iv < 0 || iv > 1) return QY265_PARAM_BAD_VALUE; c->rdoq = iv ? 2 : 0; return 0; }
    INTP("me", me, 0, 4) INTP("part", part, 0, 1) INTP("do64", do64, 0, 1) INTP("intertu", tuInter, -1, 3) INTP("intratu", tuIntra, -1, 3)
    INTP("sis", smooth, 0, 1) INTP("ts", transskip, 0, 1) INTP("subme", subme, 0, 2) INTP("merange", searchrange, 1, 512) INTP("ref", refnum, 1, 16) INTP("ref0", ref0, 1, 16)
    /* sao (qy265enc.h:143): veryfast and fast resolve to 3, which - like every level > 0 - runs this build's rule; asked for BY NAME, sao 3 is stored as 5 = the reference's own
     * decision restated (ks265_frame_cfg.sao = 2), so that the presets' streams do not pay for it (configs[0] on the MI355X: 5.5 % fewer bytes at equal PSNR-Y with the build's rule) */
    if (!strcmp(name, "sao")) { if (!num_ok || iv < 0 || iv > 4) return QY265_PARAM_BAD_VALUE; c->sao = iv == 3 ? 5 : iv; return 0; }
    /* sao-ref: the reference's decision under a name of its own - 1 = what sao 3 BY NAME selects (stored 5, ks265_frame_cfg.sao = 2), 2 = the same with its merge candidates
     * (stored 6, ks265_frame_cfg.sao = 3: sao_merge_left_flag / sao_merge_up_flag are coded), 0 = leave sao as it is */
    if (!strcmp(name, "sao-ref")) { if (!num_ok || dv != iv || iv < 0 || iv > 2) return QY265_PARAM_BAD_VALUE; if (iv) c->sao = 4 + iv; return 0; }
    INTP("wpp", enWavefront, 0, 1) INTP("fpp", enFrameParallel, 0, 1) INTP("vbv-maxrate", vbv_max_rate, 0, 10000000)
    INTP("aq", iAqMode, 0, 3)                                  /* the reference's hidden -aq (iAqMode, qy265enc.h:145) */
    INTP("denoise", vpp_denoise, 0, 3)                           /* the temporal filter on the way in (vpp_denoise / vpp_recur_filter, ks265_enc.h) */
    INTP("edge", vpp_edge, 0, 3) INTP("color", vpp_color, 0, 3)   /* edge / colour enhancement on the way in (vpp_edge / vpp_color, ks265_enc.h) */
    INTP("hdr", vpp_hdr, 0, 1)                                   /* local contrast on the way in (vpp_hdr*, ks265_enc.h); the four values below: 0 = this build's default */
    if (!strcmp(name, "hdr-iter")) { if (!num_ok || dv != iv || (iv != 0 && iv != 2 && iv != 3)) return QY265_PARAM_BAD_VALUE; c->vpp_hdr_iter = iv; return 0; }
    INTP("vbv-bufsize", vbv_buffer_size, 0, 10000000) INTP("pass", iPass, 0, 2) INTP("tlayer", temporalLayer, 0, 1) INTP("frameskip", enFrameSkip, 0, 1)
#undef INTP
    if (!strcmp(name, "fr")) { if (!num_ok || dv <= 0 || dv > 1000) return QY265_PARAM_BAD_VALUE; c->frameRate = dv; return 0; }
    if (!strcmp(name, "aqs")) { if (!num_ok || dv < 0 || dv > 3.0) return QY265_PARAM_BAD_VALUE; c->fAqStrength = dv; return 0; }   /* -aqs (fAqStrength, qy265enc.h:146) */
    if (!strcmp(name, "recur")) { if (!num_ok || !(dv >= 0) || dv > 30) return QY265_PARAM_BAD_VALUE; c->vpp_recur_filter = dv; return 0; }
    if (!strcmp(name, "hdr-strength")) { if (!num_ok || !(dv >= 0) || dv > 5) return QY265_PARAM_BAD_VALUE; c->vpp_hdr_strength = dv; return 0; }
    if (!strcmp(name, "hdr-sigma-s")) { if (!num_ok || !(dv >= 0) || dv > 100) return QY265_PARAM_BAD_VALUE; c->vpp_hdr_sigma_s = dv; return 0; }
    if (!strcmp(name, "hdr-sigma-r")) { if (!num_ok || !(dv >= 0) || dv > 100) return QY265_PARAM_BAD_VALUE; c->vpp_hdr_sigma_r = dv; return 0; }
    if (!strcmp(name, "ratetol")) { if (!num_ok || dv < 0) return QY265_PARAM_BAD_VALUE; c->fRateTolerance = dv; return 0; }
    if (!strcmp(name, "preset") || !strcmp(name, "latency") || !strcmp(name, "tune")) {
        const int k = find_name(name[0] == 'p' ? kPresetNames : name[0] == 'l' ? kLatencyNames : kTuneNames, value);
        if (k < 0) return QY265_PARAM_BAD_VALUE;
        if (name[0] == 'p') c->preset = (QY265Preset)k; else if (name[0] == 'l') c->latency = (QY265Latency)k; else c->tune = (QY265Tune)k;
        return 0;
    }
    return QY265_PARAM_BAD_NAME;
}

/* ------------------------------------------------------------------ encoder */
#define MAX_DPB 18
#define NO_PIC (-1000000)                                  /* the display index / POC of "no picture": Enc::dpb_poc, Enc::la_last_key, CtPic::disp */
#define MAX_JOBS 128                                      /* upper bound of the ring of pictures in flight; the encoder sizes its ring (Enc::ring) by picture size */
typedef struct TopWake { pthread_mutex_t mu; pthread_cond_t cv; unsigned long seq; } TopWake;
#undef MAX_INPUT                                         /* (<dirent.h> brings the terminal limit of that name along) */
#define MAX_INPUT (MAX_JOBS + 32 + 256)                /* input slots: the ring + a mini-GOP (+ in a GOP lane: a whole GOP of the next round, Enc::nin) */

typedef struct Job {
    int used, done, error;
    int disp, poc, kind, qp, nal_type, is_ref;            /* kind: 'I' 'P' 'B' */
    int gpb;                                              /* an anchor (kind 'P' for every rule of the host) that goes out as a B slice: both lists hold past anchors (`gpb`) */
    int no_sao;                                           /* the picture was coded without SAO (lean B pictures): slice_sao_luma_flag = slice_sao_chroma_flag = 0 */
    long long pts;
    int nl0, nl1, l0[4], l1[4], nrps, rps_poc[16]; unsigned char rps_used[16];
    uint8_t *cmp;                                         /* pinned host copy of the GPU's records in compact form (ks265_frame_compact_layout) */
    uint8_t *lvlbuf; uint64_t *dirty;                     /* the level planes expanded from it (plain memory) and the lines the previous picture in this slot set */
    ks265_cu8 *cu8; int16_t *lvl[3]; ks265_sao_param *sao; uint64_t *sse;      /* cu8 / sao / sse point into cmp, lvl into lvlbuf */
    int ev_err;
    uint8_t fctx[192]; int fctx_ok; int32_t *rq_host;     /* -rdoq 1: the context states the slice ended with (ks265_slice_final_contexts); the tables + lambdas the picture was quantised with (pinned) */
    long sub_seq;                                         /* this picture's number in submission order (the dispatcher's sticky device error ends at a key picture submitted after the error was seen) */
    void *wpp; ks265_slice_in sin; int started, nrows, next_row, rows_done;   /* row-wise writing of the slice (ks265_wpp_*) */
    int8_t *qp_map;                                       /* -aq: the QP of every CTU this picture was coded with (pinned; NULL without) */
    int64_t *ssim;                                        /* -ssim: per plane the sum over its 8x8 windows of llrint(ssim x 2^30) (pinned; NULL without) */
    uint32_t *hash;                                       /* `hash`: picture_crc [0..2] and picture_checksum [3..5] of the output picture's planes (pinned; NULL without) */
    uint8_t sei[48]; long sei_len;                        /* ... and the suffix SEI NAL unit a writer made of them: goes out behind the slice NAL unit, counted in no controller's bits */
    uint8_t *recon;                                       /* pinned I420 copy of the reconstruction (only with ks265_enc_set_recon_file / -md5) */
    int rslot;                                            /* `devrecon`: the slot of the lane's pool that holds the picture's packed reconstruction (travels with the picture) */
    char md5[3][33];
    void *ev;                                             /* recorded after the D2H copies */
    uint8_t *nal; size_t nal_cap; long nal_len;
    int key_headers;                                      /* parameter sets go in front of this picture */
    int rc_delta;                                         /* the controller's QP offset this picture was coded with (rate control) */
    double rc_budget;                                     /* this picture's share of the bit budget: the bitrate in force when it was handed in / frame rate (QY265EncoderReconfig) */
    double t_write_ms, t_submit, t_event, t_taken, t_done;      /* wall-clock marks: enqueued, records on the host (seen by a writer), writer started */
} Job;

/* The caller's picture has to be copied (the API gives the buffer back at once): 12 MB at 2160p, ~0.9 ms for one thread - more than the GPU needs for the
 * picture.  A few helper threads share the copy with the calling thread. */
#define COPY_HELPERS 3
typedef struct CopyPool {
    pthread_t th[COPY_HELPERS]; int nth, quit;
    pthread_mutex_t mu; pthread_cond_t cv_work, cv_done;
    struct { uint8_t *d; const uint8_t *s; size_t n; } task[COPY_HELPERS];
    unsigned posted, pending;                             /* bit k: task k waits for helper k / is not finished */
} CopyPool;
static void *copy_helper(void *arg)
{
    CopyPool *p = (CopyPool *)((void **)arg)[0]; const int k = (int)(intptr_t)((void **)arg)[1];
    free(arg);
    pthread_mutex_lock(&p->mu);
    for (;;) {
        while (!p->quit && !(p->posted & (1u << k))) pthread_cond_wait(&p->cv_work, &p->mu);
        if (p->quit) break;
        p->posted &= ~(1u << k);
        pthread_mutex_unlock(&p->mu);
        memcpy(p->task[k].d, p->task[k].s, p->task[k].n);
        pthread_mutex_lock(&p->mu);
        p->pending &= ~(1u << k);
        if (!p->pending) pthread_cond_signal(&p->cv_done);
    }
    pthread_mutex_unlock(&p->mu);
    return NULL;
}
static CopyPool *copy_pool_create(void)
{
    CopyPool *p = (CopyPool *)calloc(1, sizeof *p);
    if (!p) return NULL;
    pthread_mutex_init(&p->mu, NULL); pthread_cond_init(&p->cv_work, NULL); pthread_cond_init(&p->cv_done, NULL);
    for (int k = 0; k < COPY_HELPERS; ++k) {
        void **a = (void **)malloc(2 * sizeof *a);
        if (!a) break;
        a[0] = p; a[1] = (void *)(intptr_t)k;
        if (pthread_create(&p->th[k], NULL, copy_helper, a)) { free(a); break; }
        ++p->nth;
    }
    return p;
}
static void copy_pool_destroy(CopyPool *p)
{
    if (!p) return;
    pthread_mutex_lock(&p->mu); p->quit = 1; pthread_cond_broadcast(&p->cv_work); pthread_mutex_unlock(&p->mu);
    for (int k = 0; k < p->nth; ++k) pthread_join(p->th[k], NULL);
    pthread_mutex_destroy(&p->mu); pthread_cond_destroy(&p->cv_work); pthread_cond_destroy(&p->cv_done);
    free(p);
}
/* memcpy shared between the calling thread and the helpers (one caller at a time: the API's calling thread) */
static void copy_shared(CopyPool *p, uint8_t *d, const uint8_t *s, size_t n)
{
    if (!p || !p->nth || n < ((size_t)1 << 20)) { memcpy(d, s, n); return; }
    const size_t part = (n / (size_t)(p->nth + 1) + 4095) & ~(size_t)4095;
    size_t off = part;                                    /* the caller takes the first part */
    pthread_mutex_lock(&p->mu);
    for (int k = 0; k < p->nth && off < n; ++k, off += part) {
        p->task[k].d = d + off; p->task[k].s = s + off; p->task[k].n = n - off < part ? n - off : part;
        p->posted |= 1u << k; p->pending |= 1u << k;
    }
    pthread_cond_broadcast(&p->cv_work);
    pthread_mutex_unlock(&p->mu);
    memcpy(d, s, part < n ? part : n);
    pthread_mutex_lock(&p->mu);
    while (p->pending) pthread_cond_wait(&p->cv_done, &p->mu);
    pthread_mutex_unlock(&p->mu);
}

#define LA_RING 9                                                      /* half-size pictures kept for the analysis: the current one and eight back */
#define LA_QMAX 64                                                     /* pictures that may wait at the input for their analysis (a GOP lane runs a whole GOP ahead of its pixel path) */
#define LA_FLY 16                                                      /* analyses in flight = result areas */
/* an input slot.  i420: the pinned host copy of the picture.  key: this picture starts a closed GOP whatever the period says (GOP lanes, QY265EncoderKeyFrameRequest); base_qp: the
 * QP in force when the picture was handed in (QY265EncoderReconfig) - iper: the key period in force then - all three travel WITH the picture: the scheduler thread may be several
 * pictures behind the caller.  dev / ev_up: the slot's twin on the device, uploaded when the picture is handed in (round 4), and the event behind that upload; up_sync: the twin
 * was filled by a host-synchronous copy (nothing to wait for) */
/* Input::used, the slot's state.  Every move is made under Enc::mu (the numbers stay: 1 and 2 are what the pictures waiting and in flight are counted by):
 *   IN_FREE -> IN_ACQUIRED                the calling thread (lane_acquire): the caller writes its next picture into the slot's pinned memory; acquired again, it is the same slot
 *   IN_FREE / IN_ACQUIRED -> IN_FILLING   the calling thread (take_input_slot): the picture is on its way into the slot and its twin - the caller's own acquired slot in place,
 *                                         else a free one, else (last resort) an acquired one the caller did not use for this picture
 *   IN_FILLING -> IN_READY                the scheduler may take it: the calling thread (publish_input) without the lookahead; with it, whichever thread finds the picture's
 *                                         analysis through - the calling thread or the scheduler thread (la_publish, holding la_mu as well)
 *   IN_FILLING -> IN_FREE                 a device-library call of the way in failed: the calling thread (input_fail); the lookahead's queue is dropped whole (la_drain_locked)
 *   IN_READY -> IN_CODING                 the scheduler thread (publish_job): submitted, the twin and the pinned copy are still read
 *   IN_CODING -> IN_FREE                  the calling thread (take_output): the picture's NAL units have been handed out */
enum { IN_FREE = 0, IN_READY = 1, IN_CODING = 2, IN_FILLING = 3, IN_ACQUIRED = 4 };
typedef struct Input { int used, disp, key, base_qp, iper, mini4, kbps, la_what, la_p, la_buf, up_sync; long long pts; uint8_t *i420; uint8_t *dev; void *ev_up;
                       uint8_t *raw;                      /* a ragged lane (Enc::ragged): the picture as the caller gave it, srcW x srcH, on the device - ks265_input_pad makes `dev` of it */
                       /* `roi`: the picture's record (one int32 per CTU, ks265_roi_reduce's) on the device, its pinned twin for a map in host memory, the event behind its filling */
                       int roi_has; int32_t *roi_rec, *roi_host; void *ev_roi; } Input;

/* one pixel path: a stream (context), the frame object that codes on it, its source picture and what its quality pass and -aq write on the device.  PATH_MAIN codes every picture
 * that has no path of its own (and is the context that owns the lane's allocations and events); PATH_KEY: the key pictures (Enc::key_overlap); PATH_ANC: the anchors of the
 * pyramid GOPs (Enc::anc_on).  What only one of them has - events, counters, DPB slots, the key pictures' QP maps - stays with its owner in Enc */
enum { PATH_MAIN, PATH_KEY, PATH_ANC, NPATH };
typedef struct PixPath {
    ks265_ctx *ctx; ks265_frame *frame; ks265_pic src;
    uint64_t *dev_sse;                                    /* 64 bytes: the SSE sums of the path's latest picture */
    int64_t *dev_ssim;                                    /* -ssim: the three sums of the fused pass, 32 bytes apart inside PATH_MAIN's allocation of 96 (NULL without) */
    uint32_t *dev_hash;                                   /* `hash`: the six values of the hash pass, 32 bytes apart inside PATH_MAIN's allocation of 96 (NULL without) */
    double *aq_off, *aq_scratch; uint16_t *aq_inv;        /* -aq: the key pictures' stream has buffers of its own, the anchors share the main stream's */
} PixPath;

typedef struct Enc {
    QY265EncConfig cfg;
    int W, H, log_level;
    /* W x H is the CODED size: the caller's size rounded up to the minimum CU size (8), which is what every kernel, the lookahead, the rate control, the records and the slice
     * writers see.  srcW x srcH is the caller's (both even); ragged = they differ: pictures come in and go out at srcW x srcH (ks265_input_pad on the way in, ks265_output_crop on
     * the way out), the SPS carries the conformance window, PSNR counts the window.  crop_scr: the scratch picture ks265_enc_get_device_recon crops into (a ragged lane with
     * `devrecon`: made at open); ev_crop: recorded behind the conversion that read it last, in that call's stream - the next call's crop, in whatever stream, waits for it (crop_used) */
    int srcW, srcH, ragged; uint8_t *crop_scr; void *ev_crop; int crop_used;
    CopyPool *pool;                                       /* shared by the lanes of one handle (owned by it) */
    int me_method, hex_thr, subme, refs, use_sao, use_df, gop_b, hier;                  /* resolved tools */
    int lean_b;                                                                         /* B pictures nothing predicts from: no intra candidates, no joint refinement, no SAO (KS265_LEAN_B=0: as the others) */
    int gpb;                                                                            /* `gpb` in force: an anchor that searches two or more past anchors is coded as a B slice (gop_plan) */
    int refs0;                                                                          /* -ref0 (qy265enc.h:142, the reference's ActiveRefNumFrm0InGop): how many past anchors an anchor of the pyramid searches */
    int base_qp, iper, nthreads;
    PixPath path[NPATH]; ks265_frame_geom geom; ks265_frame_cfg fcfg; ks265_stream_cfg scfg;
    /* device: three streams - copy-in (ctx_in), the pixel path (path[].ctx), copy-out (ctx_out) - so that the H2D of picture n+1 and the D2H of
     * picture n-1 run under the kernels of picture n.  Hand-over by events only (no host thread blocks): input buffers and output staging
     * sets rotate over NPIPE slots. */
#define NPIPE 3
    ks265_ctx *ctx_in, *ctx_out;
    uint8_t *dev_in[NPIPE]; void *ev_h2d[NPIPE], *ev_loaded[NPIPE];
    void *spacer[64]; int nspacer;
    /* round 6: the caller's planes are pinned in place (ks265_host_register, cached by address) and uploaded by DMA straight into the slot's device twin - no copy into pinned memory of
     * the encoder's own (KS265_INPUT_COPY=1: the copying path; pictures under 1 MB always copy).  The upload is waited for before QY265EncoderEncodeFrame returns - the SDK's own callers
     * refill ONE buffer for every picture (encoderwrapper.c:367-379) - unless KS265_INPUT_HOLD=1 (the caller keeps every buffer until its picture has come out, qy265enc.h:153-156) */
    int direct_in, hold_in; ks265_ctx *ctx_upl; struct Input *pending_up;
    int dev_id, dev_in_on;                                /* the lane's GPU; ks265_enc_enable_device_input: every input slot has a twin, pictures may come from device memory */
    ks265_ctx *ctx_up;                                    /* with the lookahead: = ctx_la, the stream the caller's thread feeds with uploads (the moment a picture is handed in) and with the analysis; else NULL */
    uint8_t *stg[NPIPE]; size_t cmp_off[8];               /* staging blocks of the (compact) records on the device and their layout */
    void *ev_staged[NPIPE], *ev_drained[NPIPE];
    /* split pipeline (default): the source picture of slot k is unpacked and padded on the copy-in stream into srcq[k], and the picture's drain (SSE, packing of the
     * records) runs on the copy-out stream behind ev_coded[k]; the next picture's search does not wait for either - it waits for ev_packed[k] only where it first writes
     * a record (ks265_frame_set_records_fence).  Measured at 2160p IPPP: 120 us of a 1.11 ms picture period leave the critical path. */
    /* -aq N (iAqMode != 0): adaptive quantisation = the reference's calcFrameAdaptQuant enc@0x4653c0 on the source picture (ks265_frame_adapt_quant, pinned on recorded
     * calls), one QP per CTU from it (ks265_aq_ctu_map), the pixel path and the writer on that map (ks265_frame_set_qp_map, cu_qp_delta) */
    int aq_on, aq_nx, aq_ny; int8_t *dev_qmap[NPIPE], *dev_qmap_key[2];   /* dev_qmap_key: the key pictures' stream (its own maps, rotating with nkeys: a key picture runs beside the pictures of its rotation slot) */
    int zero_latency;                                     /* -latency zerolatency without B pictures / lookahead / lanes: every EncodeFrame call hands out its own picture */
    int copy_mb;                                          /* KS265_COPYOUT_MB = N: hipMemcpyAsync takes the fixed part + N MB of stored lines per P / B picture (a key picture: everything) and the copy kernel
                                                           * only what lies beyond; default -1 = the copy kernel alone.  On this runtime the D2H hipMemcpyAsync is itself a kernel (__amd_rocclr_copyBuffer,
                                                           * 110 us for 4 MB): no better neighbour than ours (50 us for the ~2 MB a picture really holds) - measured both ways, within +- 1.5 % */
    int split; ks265_pic srcq[NPIPE]; void *ev_coded[NPIPE], *ev_packed[NPIPE];
    long seq;                                             /* pictures submitted */
    /* single-reference P pictures and B pictures as graphs: the launch sequence of a picture (unpack, the pixel path, SSE, packing of the records: ~20 launches) only
     * depends on a few rotating device pointers, the QP and two bits of frame state; each combination is captured once and replayed with one runtime call */
#define MAX_GRAPHS 256
    int use_graph, ngraph; struct { uint64_t key[9]; void *exec; } graph[MAX_GRAPHS];
    /* `devrecon` (ks265_enc.h): a pool of packed-I420 pictures on the device, one slot per picture from its submission until the call after the one that handed it out
     * (ks265_recon.h keeps the books, under mu).  ev_packed: behind the pack on the picture's stream; ev_read: behind the last conversion that read the slot (read_on: there
     * was one) - the next pack into the slot waits for it.  ctx_rec: the context the conversions run on (the calling thread's alone: it adopts the caller's stream).  taken: what take_output just moved out
     * of the ring, for the caller of take_output (the calling thread) to hand out or stash */
    int roi_on;                                           /* `roi` (ks265_enc.h): pictures may come with a map of quantiser offsets; one QP per CTU in the stream */
    /* `analysis` (ks265_enc.h): the same pool, the same slot numbers - a slot owns a reconstruction if devrecon is on and an analysis block (an: ks265_analysis_bytes) if analysis
     * is on; pool_on: either.  ev_packed is recorded once, behind the picture's last pack; each fetch kind has its own read event (ev_read_an / read_on_an: the exports) */
    int devrecon, analysis, pool_on, lane_idx; ReconPool rpool;
    struct ReconSlot { uint8_t *dev; void *ev_packed, *ev_read; int read_on; uint8_t *an; void *ev_read_an; int read_on_an; } rslot[RECON_POOL_MAX];
    ks265_ctx *ctx_rec; ReconList taken;
    int recon_fd, recon_on; uint8_t *dev_recon;           /* reconstruction dump (the CLI's -o) and / or plane MD5s (-md5 1): recon_on = the pictures come back to the host */
    int md5, fixqp, psnr_hdr; int md5_next; char (*md5_ring)[3][33]; unsigned char *md5_have;   /* MD5 lines go out in display order (ring of 256 by display index) */
    ks265_pic dpb[MAX_DPB]; int dpb_poc[MAX_DPB]; int ndpb;
    /* -ssim: the fused pass is there and asked for (its device sums: PixPath::dev_ssim); the session's
     * totals in output order as exact integers (hi x 2^30 + lo: the same for any number of GOP lanes), the picture accounted last and when (q_seq: across lanes) */
    int hash_on;                                          /* `hash` in force (2 CRC, 3 checksum) and the hash pass is there: every picture is followed by its decoded picture hash SEI message */
    int ssim_on; long long q_hi[3], q_lo[3]; int q_last_poc; double q_last_sse[3], q_last_ssim[3]; unsigned long q_seq;
    /* key pictures on their own stream and frame object (path[PATH_KEY]): an intra picture keeps 34 of 256 compute units busy for ~26 ms (2160p); coded as soon as its
     * input arrives - the pixel path is tens of pictures behind the input - it runs underneath the P pictures of the previous GOP instead of between
     * two GOPs.  Its reconstruction goes to one of two DPB slots of its own; the first P picture of the GOP waits for ev_key. */
    int refs_b;                                           /* reference pictures per list of a pyramid's B pictures (1 .. 4) */
    /* round 5 - the ANCHOR LANE of the pyramid GOPs: a mini-GOP's anchor P picture predicts from the anchor before it and from nothing else, so the chain of anchors is coded on a
     * stream and frame object of its own (path[PATH_ANC], like the key pictures), ahead of the B pictures of the mini-GOPs behind it: its kernels - and the long intra chain pass of a picture
     * 4 or 8 away from its reference - run beside the B pictures' instead of in front of them.  Four DPB slots of its own, rotating; a slot is overwritten only after the B
     * pictures that read its previous content have run on the main stream (ev_mg: one mark per mini-GOP, recorded behind its last B picture) */
    int anc_on, nanch, last_on_anc; void *ev_anc, *ev_mg[8];
    int key_overlap, nkeys; void *ev_key, *ev_firstp[2];
    /* scheduling */
    Input in[MAX_INPUT]; int nin, next_disp, in_disp;          /* next_disp: pictures handed to the scheduler; in_disp: pictures taken in (= next_disp + the lookahead's queue la_q) */
    GopRules rules; GopState gs;                          /* ks265_gop.h: what the planner reads of the resolved tools (lane_resolve fills it last), and what it carries from unit to unit */
    int coded_upto;                                       /* display index up to which everything is scheduled */
    int force_key;
    int gop_end, gop_end_seen;                            /* GOP lanes: display index of the last picture of a GOP that ended early (-1: none); what the scheduler has acted on */
    int multi;                                            /* one of several GOP lanes of a handle */
    /* scene-cut lookahead (-lookahead N > 0; SURVEY.md 8(f) rank 2, scenecut enc@0x47e9d0 lineage): a stream and a frame object of HALF the size of their own; every
     * input picture is compared with its predecessor before the scheduler sees it (ks265_lookahead_picture: per 8x8 block of the half-size picture the intra
     * pre-selection cost against the integer-search cost) - where prediction from the previous picture is not clearly cheaper than intra coding a closed GOP starts */
    int la_on, la_have_prev, la_last_key, la_w, la_h; long la_cuts, la_mini4;
    int mg_adapt;                                                     /* slice-type decision (-lookahead N with the hierarchical GOP): a block of 8 pictures is coded as 8 or as 4 + 4 */
    long long la_prev_icost;                                           /* -scenecut N: the previous picture's intra cost (-1: none yet) */
    unsigned long long la_c4_prev;                                     /* inter cost of the previous picture on the GOP's grid of 4 against the picture 4 back */
    int la_auto;                                                       /* no -lookahead given, hierarchical GOP: the slice-type decision alone (pictures on the GOP's grid of 4), no scene cuts - works in GOP lanes */
    double la_t_bp, la_t_take, la_t_wait; long la_n_wait, la_n_poll;       /* where the caller's time goes (log level 1) */
    pthread_mutex_t la_mu;                                             /* the queue below and the decisions' state: the caller's thread fills it, the caller's and the scheduler's threads empty it (lock order: la_mu, then mu) */
    struct Input *la_q[LA_QMAX]; int la_qn, la_flying, la_seq, la_keep; void *la_evs[LA_FLY];   /* pictures handed in and not yet with the scheduler (display order); analyses in flight; their events / result areas, round robin */
    ks265_ctx *ctx_la; ks265_frame *frame_la; ks265_frame_geom geom_la; ks265_pic la_pic[LA_RING];
    uint32_t *la_cost_ws; uint64_t *la_dev_out, *la_host_out;
    /* cuTree (-rc 3 with -cutree 1, the default; round 6): the reference's macroblock-tree over the lookahead window.  Before a key picture / a mini-GOP is
     * submitted the scheduler thread runs, on a stream of its own, the reference's calcFrameCost enc@0x4a7410 (ks265_calc_frame_cost) for every picture of the window against the
     * pictures it will be predicted from, cuTreePropagate enc@0x47d460 from the window's end back to the mini-GOP (reverse coding order, as CInputPicManage::updateQueue does), and the
     * finish (enc@0x480964: offset = AQ offset - 1.8 log2((propagated + intra') / intra')) for the pictures about to be coded; their QP per CTU = picture QP + the mean of the CTU's
     * block offsets (ks265_qoff_ctu_map), through the -aq plumbing (ks265_frame_set_qp_map, cu_qp_delta).  Costs are cached per picture and reference pair. */
#define CT_RING 128
    int ct_on, ct_lg, ct_nx, ct_ny, ct_w, ct_h, ct_stride, ct_pad, ct_depth, ct_preset, qmap_on, qmap_fd;
    struct CtPic { int disp, p0, p1, intra_done, used; uint8_t *blk, *low; uint16_t *intra, *invq, *prop, *inter; uint8_t *imode, *bits; int32_t *mv0, *c0, *mv1, *c1; double *aq_off, *qoff; ks265_cfc_sums *sums; void *ev_used; } ct[CT_RING];
    ks265_ctx *ctx_ct; void *ct_ws, *ct_ev; uint64_t *ct_acc; double *ct_scratch; uint8_t *ct_full;
    /* decisions that only the steps of lane_open and lane_close read (lane_resolve) */
#define UPL_NONE 99
    struct {
        int la_wanted, la_order, la_prio;                 /* the lookahead's stream: asked for; created first (0), behind the copy streams (1), else with the lookahead's objects; KS265_LA_PRIO */
        int upl_at;                                       /* the uploads' stream: created at position -1 / 0 / 1 / 2 (open_upl_stream), UPL_NONE: there is none */
        int key_prio, anc_prio, srcq;                     /* stream priorities of the two paths beside the main one; the split pipeline's source pictures are allocated */
        int recon_slots;                                  /* `devrecon`: slots of the pool */
        int input_slots, pinned_mb; size_t spacer;        /* KS265_INPUT_SLOTS (or ENV_UNSET), KS265_PINNED_MB; KS265_PIC_SPACER: bytes in front of every picture (pic_alloc) */
        const char *qmap_path;                            /* KS265_DUMP_QPMAP */
    } plan;
    struct TopWake *wake;                                 /* lanes: the handle's caller sleeps here until a picture of ANY lane is finished */
    Job jobs[MAX_JOBS]; int ring, job_head, job_tail, njobs;   /* ring of `ring` pictures in coding order */
    /* workers */
    pthread_t th[64]; int nth; pthread_mutex_t mu; pthread_cond_t cv_work, cv_done; int quit;
    int next_work, npending;                              /* ring index of the next job to write, jobs whose records are on the host but not yet taken by a writer */
    pthread_t disp; int disp_on; pthread_cond_t cv_disp; int next_ready, nwait;   /* the one thread that waits for GPU events (in submission order) */
    /* the scheduler thread: GOP decisions + every GPU enqueue of a picture (some thirty runtime calls) happen here, not on the caller's thread */
    pthread_t sched; int sched_on; pthread_cond_t cv_sched, cv_sched_done; int sched_seen, sched_flush, sched_idle, sched_err;
    int dev_err; long dev_err_seq;                        /* sticky device error of the lane (dispatcher), and how many pictures had been submitted when it was seen */
    struct WorkerArg { struct Enc *e; int idx; } warg[64];
    /* output */
    QY265Nal nals[4 * MAX_JOBS + 8]; uint8_t *hdr; long hdr_len, hdr_part[3];
    uint8_t *outbuf; size_t outcap, outpos;               /* NAL payloads handed to the caller live here until the next call */
    ks265_enc_stats st;
    /* rate control (frame level, rc 1 / 2 / 4): the QP offset of a mini-GOP is a closed-form function of the pictures coded at least RC_LAG pictures earlier
     * (coding order) - the scheduler waits for exactly those, so the stream does not depend on thread timing.  rc_qp_delta belongs to the scheduler thread;
     * the sums are updated under mu in coding order (rc_account) */
#define RC_LAG 16
#define RC_HIST 512
    /* -rdoq 1 (the reference's rdoQuant in the pixel path, round 6): its bit tables follow the stream - a P / B picture is quantised with the tables built from the context states of
     * the latest picture of its kind that was coded at least RC_LAG + 1 pictures earlier (rq_hist: tables per accounted picture, like rc_hist: what a picture is coded with does
     * not depend on how fast the writers were), else from the initial states of its slice type at its QP; Job::rq_host: the picture's tables + lambdas, pinned */
#define RQ_HIST 64
    int rdoq_on; int32_t *rq_hist; char rq_hist_kind[RQ_HIST]; int64_t rq_lam[104]; long rq_gop_seq;   /* rq_gop_seq: the submission number of the current GOP's key picture - tables never cross a key picture (closed GOPs: the stream does not depend on how GOPs are dealt to lanes) */
    double rc_sum_norm, rc_hist[RC_HIST]; long rc_acc_seq, rc_sub; int rc_acc_idx; int rc_qp_delta;
    double rc_sum_budget, rc_bhist[RC_HIST], rc_sum_real, rc_rhist[RC_HIST];   /* the budget and the bits really produced, summed picture by picture like rc_sum_norm */
    /* ks265_enc_enable_device_scale: device pictures of other sizes are scaled into the slot's twin (ks265_input_scale on ctx_up, where ks265_input_convert stands).  sc_scratch: the
     * RGB sources' I420 picture at the largest source size; sc_plan: the lane's plans by (source size, filter), the least recently used one replaced (a picture's plan reaches
     * lane_put as an argument, `sc`).  Behind every other field: the layout in front of them is the one the lanes have always had */
#define SCALE_PLANS 4
    int sc_on, sc_max_w, sc_max_h; uint8_t *sc_scratch; long sc_tick;
    struct ScalePlan { ks265_scale_plan *plan; int sw, sh, filter; long used; } sc_plan[SCALE_PLANS];
    /* `vpp_denoise` / `vpp_recur_filter` (lane_resolve: dn_on, dn_cfg): two history pictures of the coded size on the lane's device, used ping-pong by stage_denoise -
     * dn_hist[dn_at] holds the last filtered picture once dn_has is set.  Off: no field is touched, nothing is allocated */
    int dn_on, dn_at, dn_has; ks265_denoise_cfg dn_cfg; uint8_t *dn_hist[2];
    /* `vpp_edge` / `vpp_color` (lane_resolve: en_on, en_cfg; stage_enhance).  en_luma: the W x H copy of the luma that the stencil reads, owned by a lane with vpp_edge on and
     * the denoiser off or vpp_hdr on (with the denoiser alone, the history picture it just wrote is that copy).  Off: no field is touched, nothing is allocated */
    int en_on; ks265_enhance_cfg en_cfg; uint8_t *en_luma;
    /* `vpp_hdr` (lane_resolve: hdr_on, hdr_cfg; stage_hdr).  hdr_work: the filter's work buffer, ks265_input_hdr_work_bytes (hdr_bytes) of the coded size, one per lane.  With
     * it on, stage_enhance reads en_luma whether the denoiser runs or not (the history picture is no longer the luma in front of the enhancement).  Off: no field is touched,
     * nothing is allocated */
    int hdr_on; ks265_hdr_cfg hdr_cfg; size_t hdr_bytes; void *hdr_work;
    /* ks265_enc_enable_tonemap: a device picture of 10 to 16 bits in 4:2:0 goes through ks265_input_tonemap where ks265_input_convert stands (stage_device), with the lane's
     * own plan - the tables in device memory, made by the enabling call and destroyed at close.  The filter has no state.  Off: no field is touched, nothing is allocated */
    int tm_on; ks265_tonemap_plan *tm_plan;
} Enc;

static ks265_ctx *main_ctx(const Enc *e) { return e->path[PATH_MAIN].ctx; }
static ks265_frame *main_frame(const Enc *e) { return e->path[PATH_MAIN].frame; }
static double now_ms(void) { struct timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return t.tv_sec * 1e3 + t.tv_nsec * 1e-6; }
static void rc_account(Enc *e);
static void lane_wake_top(Enc *e)
{
    TopWake *w = e->wake;
    if (!w) return;
    pthread_mutex_lock(&w->mu); ++w->seq; pthread_cond_broadcast(&w->cv); pthread_mutex_unlock(&w->mu);
}
static int lane_recon_on(Enc *e);
static int hip_rc(int r) { return r == 0 ? QY_OK : r == KS265_OUTOFMEMORY ? QY_OUTOFMEMORY : r == KS265_POINTER ? QY_POINTER : r == KS265_NOTSUPPORTED ? QY_NOTSUPPORTED : QY_FAIL; }

static int pic_alloc(Enc *e, ks265_pic *p)
{
    /* KS265_PIC_SPACER = bytes: an unused allocation in front of every picture (where pictures lie against each other in device memory decides what shares a memory channel:
     * round 4) */
    if (e->plan.spacer && e->nspacer < 64) { void *d = NULL; if (!ks265_dev_malloc(main_ctx(e), &d, e->plan.spacer)) e->spacer[e->nspacer++] = d; }
    int r = ks265_dev_malloc(main_ctx(e), (void **)&p->y, (size_t)e->geom.bytes_y);
    if (!r) r = ks265_dev_malloc(main_ctx(e), (void **)&p->u, (size_t)e->geom.bytes_c);
    if (!r) r = ks265_dev_malloc(main_ctx(e), (void **)&p->v, (size_t)e->geom.bytes_c);
    return r;
}
static void pic_free(Enc *e, ks265_pic *p) { ks265_dev_free(main_ctx(e), p->y); ks265_dev_free(main_ctx(e), p->u); ks265_dev_free(main_ctx(e), p->v); p->y = p->u = p->v = NULL; }

/* ---- the dispatcher: ONE host thread waits for the pictures' events, in submission order (the copy-out stream finishes them in that order), and
 *      releases them to the writers.  Writers that waited inside the GPU runtime themselves would contend with the calling thread's enqueues. */
static void *dispatcher(void *arg)
{
    Enc *e = (Enc *)arg;
    pthread_mutex_lock(&e->mu);
    for (;;) {
        while (!e->quit && e->nwait == 0) pthread_cond_wait(&e->cv_disp, &e->mu);
        if (e->quit) break;
        Job *j = &e->jobs[e->next_ready];
        pthread_mutex_unlock(&e->mu);
        int err = 0;
        err = ks265_event_wait(e->ctx_out, j->ev);
        /* the device error word of the streams that code pictures (a wavefront that timed out leaves a picture whose levels do not match its reconstruction): the
         * picture - this one or one enqueued after it - fails instead of going out as if nothing had happened */
        if (!err) err = ks265_take_device_error(main_ctx(e));
        if (!err && e->path[PATH_KEY].ctx) err = ks265_take_device_error(e->path[PATH_KEY].ctx);
        if (err) logf_(2, e->log_level, "ks265enc: device error at picture %d: %s\n", j->disp, "intra wavefront timeout or device error flag (ks265_take_device_error)");
        j->t_event = now_ms();
        pthread_mutex_lock(&e->mu);
        /* the error word does not say WHICH picture raised it: it may be one enqueued after this one (a key picture running ahead on its own stream), and every picture
         * predicted from a broken reconstruction is broken too.  So the error sticks to the lane: this picture and all that were already submitted when it was seen fail,
         * and so does everything after them up to the first key picture (IDR: a closed GOP) submitted later */
        if (err && !e->dev_err) { e->dev_err = err; e->dev_err_seq = e->rc_sub; }
        else if (!err && e->dev_err) { if (j->kind == 'I' && j->sub_seq >= e->dev_err_seq) e->dev_err = 0; else err = e->dev_err; }
        j->ev_err = err;
        e->next_ready = (e->next_ready + 1) % e->ring; --e->nwait; ++e->npending;
        pthread_cond_broadcast(&e->cv_work);
    }
    pthread_mutex_unlock(&e->mu);
    return NULL;
}

/* ---- slice writers.  Every picture is written as CTU-row substreams (entropy_coding_sync, the reference's WPP: ks265_wpp_*).  A writer thread takes
 *      the next picture and codes its rows one after the other - pictures of a GOP in parallel, no waiting inside a picture.  A key picture's slice is
 *      an order of magnitude longer than a P picture's and output is in coding order, so writers that look for work JOIN a key picture that is in
 *      progress before they start another picture: its rows
 *      are handed out in ascending order, each row runs at most two CTUs behind the row above (the wavefront of qy265executeEncCtuTaskWpp enc@0x475d20). */
/* the level planes of one CTU row of a picture from its compact records: clear the lines the previous picture in this job slot had set there, put this
 * picture's lines in place.  Done by the thread that writes the row (rows of a key picture by different threads); a line that straddles two CTU rows is
 * written twice with the same bytes.  ctu_row < 0: the whole picture. */
static void expand_levels(Enc *e, Job *j, int ctu_row)
{
    const size_t npx = (size_t)e->W * e->H, pb[3] = {npx * 2, npx / 2, npx / 2};
    uint8_t *plane[3] = {(uint8_t *)j->lvl[0], (uint8_t *)j->lvl[1], (uint8_t *)j->lvl[2]};
    size_t first[4]; first[0] = 0;
    for (int p = 0; p < 3; ++p) first[p + 1] = first[p] + (pb[p] + 63) / 64;
    const uint32_t *table = (const uint32_t *)(j->cmp + e->cmp_off[4]);
    const uint64_t *bm = (const uint64_t *)(j->cmp + e->cmp_off[5]);
    const uint8_t *data = j->cmp + e->cmp_off[6];
    for (int p = 0; p < 3; ++p) {
        /* byte range of the CTU row in this plane -> line range */
        const size_t rowb = (size_t)(p ? e->W / 2 : e->W) * 2, rows = (size_t)(p ? e->H / 2 : e->H), ch = p ? 32 : 64;
        size_t y0 = ctu_row < 0 ? 0 : (size_t)ctu_row * ch, y1 = ctu_row < 0 ? rows : y0 + ch;
        if (y1 > rows) y1 = rows;
        if (y0 >= y1) continue;
        const size_t l0 = first[p] + y0 * rowb / 64, l1 = first[p] + (y1 * rowb + 63) / 64;
        for (int pass = 0; pass < 2; ++pass)                           /* 0: clear the old lines, 1: place the new ones */
            for (size_t w = l0 / 64; w <= (l1 - 1) / 64; ++w) {
                uint64_t bits = pass ? bm[w] : j->dirty[w];
                if (w == l0 / 64) bits &= ~0ull << (l0 & 63);
                if (w == (l1 - 1) / 64 && (l1 & 63)) bits &= ~0ull >> (64 - (l1 & 63));
                if (!bits) continue;
                size_t k = 0;
                if (pass) {                                            /* rank of the word's first line in the data area: chunk base + lines of the chunk's earlier words */
                    k = (size_t)table[w / 16];
                    for (size_t q = w & ~(size_t)15; q < w; ++q) k += (size_t)__builtin_popcountll(bm[q]);
                    k += (size_t)__builtin_popcountll(bm[w] & ~bits & ((bits & (~bits + 1)) - 1));      /* lines of this word below the range */
                }
                while (bits) {
                    const int b = __builtin_ctzll(bits);
                    bits &= bits - 1;
                    const size_t L = w * 64 + (size_t)b;
                    const size_t off = (L - first[p]) * 64, n = pb[p] - off < 64 ? pb[p] - off : 64;
                    if (pass) memcpy(plane[p] + off, data + (k++) * 64, n); else memset(plane[p] + off, 0, n);
                }
            }
    }
}

static Job *find_helpable(Enc *e)
{
    for (int i = 0, k = e->job_head; i < e->njobs; ++i, k = (k + 1) % e->ring) {
        Job *j = &e->jobs[k];
        if (j->used && j->started && !j->done && j->kind == 'I' && j->next_row < j->nrows) return j;
    }
    return NULL;
}
static void *worker(void *arg)
{
    Enc *e = ((struct WorkerArg *)arg)->e;
    pthread_mutex_lock(&e->mu);
    for (;;) {
        Job *j = NULL;
        int owner = 0;
        while (!e->quit) {
            /* a key picture in progress comes first: output is in coding order, everything coded after it waits for its slice */
            if ((j = find_helpable(e)) != NULL) break;
            if (e->npending > 0) { j = &e->jobs[e->next_work]; e->next_work = (e->next_work + 1) % e->ring; --e->npending; owner = 1; break; }
            pthread_cond_wait(&e->cv_work, &e->mu);
        }
        if (e->quit) break;
        if (owner) {
            pthread_mutex_unlock(&e->mu);
            j->t_taken = now_ms();
            int err = j->ev_err;                                 /* the dispatcher saw this picture's records reach the host */
            if (!err && e->recon_fd >= 0 && j->recon) {
                const size_t fsz = (size_t)e->srcW * e->srcH * 3 / 2;
                if (e->ragged) {                                         /* the window, as a decoder writes it */
                    uint8_t *win = (uint8_t *)malloc(fsz);
                    if (win) ks265_recon_crop(j->recon, e->W, e->H, e->srcW, e->srcH, win);
                    if (!win || pwrite(e->recon_fd, win, fsz, (off_t)j->disp * (off_t)fsz) != (ssize_t)fsz) err = KS265_FAIL;
                    free(win);
                } else
                if (pwrite(e->recon_fd, j->recon, fsz, (off_t)j->disp * (off_t)fsz) != (ssize_t)fsz) err = KS265_FAIL;
            }
            if (!err && e->md5 && j->recon) {
                const size_t np = (size_t)e->W * e->H;
                md5_hex(j->recon, np, j->md5[0]); md5_hex(j->recon + np, np / 4, j->md5[1]); md5_hex(j->recon + np + np / 4, np / 4, j->md5[2]);
            }
            if (!err) {
                ks265_slice_in *s = &j->sin;
                memset(s, 0, sizeof *s);
                s->nal_type = j->nal_type; s->slice_type = j->kind == 'I' ? KS265_SLICE_I : j->kind == 'P' && !j->gpb ? KS265_SLICE_P : KS265_SLICE_B;
                s->poc = j->poc; s->qp = j->qp; s->num_rps = j->nrps;
                memcpy(s->rps_poc, j->rps_poc, sizeof s->rps_poc); memcpy(s->rps_used, j->rps_used, sizeof s->rps_used);
                s->num_l0 = j->nl0; s->num_l1 = j->nl1; memcpy(s->l0_poc, j->l0, sizeof s->l0_poc); memcpy(s->l1_poc, j->l1, sizeof s->l1_poc);
                s->cu8 = j->cu8; s->lvl[0] = j->lvl[0]; s->lvl[1] = j->lvl[1]; s->lvl[2] = j->lvl[2]; s->sao = e->use_sao && !j->no_sao ? j->sao : NULL;
                s->qp_map = e->qmap_on ? j->qp_map : NULL;
                if (e->qmap_on && e->qmap_fd >= 0) {                     /* KS265_DUMP_QPMAP=file (tests): display index, kind, QP, CTU count, then the map - one record per picture, whole records only */
                    const int nct = e->geom.ctu_cols * e->geom.ctu_rows;
                    uint8_t *rec = (uint8_t *)malloc(16 + (size_t)nct);
                    if (rec) { const int32_t hd[4] = {j->disp, j->kind, j->qp, nct}; memcpy(rec, hd, 16); memcpy(rec + 16, j->qp_map, (size_t)nct); if (write(e->qmap_fd, rec, 16 + (size_t)nct) < 0) { /* diagnostics only */ } free(rec); }
                }
                err = ks265_wpp_begin(&e->scfg, s, j->wpp);
            }
            pthread_mutex_lock(&e->mu);
            j->t_write_ms = 0;
            if (err) {                                           /* nothing to write: the picture is finished (with its error) */
                j->error = err; j->done = 1;
                rc_account(e);
                pthread_cond_broadcast(&e->cv_done); lane_wake_top(e);
                continue;
            }
            j->nrows = ks265_wpp_rows(j->wpp); j->next_row = 0; j->rows_done = 0; j->started = 1;
            if (j->kind == 'I') pthread_cond_broadcast(&e->cv_work);   /* idle writers may join */
        }
        while (j->next_row < j->nrows) {
            const int row = j->next_row++;
            pthread_mutex_unlock(&e->mu);
            const double t0 = now_ms();
            expand_levels(e, j, row);
            (void)ks265_wpp_code_row(j->wpp, row);               /* a failure is kept in the job memory and reported by ks265_wpp_finish */
            const double dt = now_ms() - t0;
            pthread_mutex_lock(&e->mu);
            j->t_write_ms += dt;
            if (++j->rows_done == j->nrows) {                    /* the thread that finishes the last row assembles the NAL unit */
                pthread_mutex_unlock(&e->mu);
                const double t1 = now_ms();
                const size_t need = ks265_wpp_nal_bound(j->wpp);          /* an incompressible picture at a low QP costs more than two bytes per sample: the buffer follows the writer's own bound */
                int oom = 0;
                if (need > j->nal_cap) {
                    uint8_t *nb = (uint8_t *)realloc(j->nal, need);
                    if (nb) { j->nal = nb; j->nal_cap = need; } else oom = 1;
                }
                const long n = oom ? (long)KS265_OUTOFMEMORY : ks265_wpp_finish(j->wpp, j->nal, j->nal_cap);
                /* `hash`: the picture's decoded picture hash SEI message, a NAL unit of its own behind the slice's (the six values came home in front of the picture's event) */
                j->sei_len = e->hash_on && n >= 0 ? ks265_write_picture_hash_sei(e->hash_on - 1, j->hash + (e->hash_on == 2 ? 0 : 3), j->sei, sizeof j->sei) : 0;
                j->fctx_ok = e->rdoq_on && n >= 0 && ks265_slice_final_contexts(&e->scfg, j->wpp, j->fctx, (int)sizeof j->fctx, NULL) > 0;
                memcpy(j->dirty, j->cmp + e->cmp_off[5], e->cmp_off[6] - e->cmp_off[5]);      /* what the next picture in this slot has to clear */
                pthread_mutex_lock(&e->mu);
                j->t_write_ms += now_ms() - t1;
                j->nal_len = n; j->error = n < 0 ? (int)n : j->sei_len < 0 ? (int)j->sei_len : 0; j->done = 1; j->t_done = now_ms();
                rc_account(e);
                pthread_cond_broadcast(&e->cv_done); lane_wake_top(e);
            }
        }
    }
    pthread_mutex_unlock(&e->mu);
    return NULL;
}

/* rate control: account finished pictures in coding order (under mu; called where a picture becomes done and before its ring slot is freed).  A picture's bits
 * are normalised to the base QP with the 6-steps-per-octave rule (bits x 2^(delta / 6)), so the sums say what the stream would have cost without the
 * controller.  rc_hist keeps the running sum after every picture: the decision for picture n reads the entry of picture n - RC_LAG - 1 whatever has been
 * accounted since (pictures finish early or late; the decision must not depend on that). */
static void rc_account(Enc *e)
{
    while (e->rc_acc_seq < e->rc_sub) {
        Job *j = &e->jobs[e->rc_acc_idx];
        if (!j->used || !j->done) break;
        if (e->rdoq_on) {                                         /* the tables this picture's final states give, for the pictures of its kind RC_LAG and more pictures on */
            const int slot = (int)(e->rc_acc_seq % RQ_HIST);
            e->rq_hist_kind[slot] = 0;
            if (j->fctx_ok && !j->error && ks265_rdoq_tables(&e->scfg, j->fctx, 0, 0, e->rq_hist + (size_t)slot * 1440) == 0) e->rq_hist_kind[slot] = (char)j->kind;
        }
        e->rc_sum_norm += (double)(j->nal_len > 0 ? j->nal_len : 0) * 8.0 * exp2((double)j->rc_delta / 6.0);
        e->rc_hist[e->rc_acc_seq % RC_HIST] = e->rc_sum_norm;
        e->rc_sum_budget += j->rc_budget; e->rc_bhist[e->rc_acc_seq % RC_HIST] = e->rc_sum_budget;      /* per picture at the bitrate it was handed in with: a later
                                                                                                           * QY265EncoderReconfig does not re-price the past */
        e->rc_sum_real += (double)(j->nal_len > 0 ? j->nal_len : 0) * 8.0; e->rc_rhist[e->rc_acc_seq % RC_HIST] = e->rc_sum_real;
        e->rc_acc_idx = (e->rc_acc_idx + 1) % e->ring; ++e->rc_acc_seq;
    }
}
/* scheduler thread: the offset for the pictures submitted next.  Waits until every picture up to RC_LAG before the next one is written (the writers do not need
 * the caller for that), then delta = 6 log2(normalised bits / budget) over exactly those pictures, at most 4 steps away from the previous value. */
static int rc_decide(Enc *e)
{
    if (!(e->cfg.rc == 1 || e->cfg.rc == 2 || e->cfg.rc == 4)) return 0;
    pthread_mutex_lock(&e->mu);
    const long need = e->rc_sub - RC_LAG;                              /* pictures [0, need) decide */
    for (;;) {
        rc_account(e);
        if (e->rc_acc_seq >= need || e->quit) break;
        pthread_cond_wait(&e->cv_done, &e->mu);
    }
    int d = e->rc_qp_delta;
    if (need >= 4 && !e->quit) {
        const double spent = e->rc_hist[(need - 1) % RC_HIST], budget = e->rc_bhist[(need - 1) % RC_HIST], real = e->rc_rhist[(need - 1) % RC_HIST];
        if (spent > 0 && budget > 0) {
            /* model term: what the stream costs at the base QP against the budget, 6 QP steps per octave; feedback term: the bits really produced so far against the
             * budget so far (half weight, at most 2 steps) - where the content's rate does not halve every 6 steps the model term alone settles beside the target */
            double fb = need >= 32 && real > 0 ? 3.0 * log2(real / budget) : 0.0;
            fb = fb > 2.0 ? 2.0 : fb < -2.0 ? -2.0 : fb;
            int want = (int)lrint(6.0 * log2(spent / budget) + fb);
            if (want > d + 4) want = d + 4;
            if (want < d - 4) want = d - 4;
            d = want < -51 ? -51 : want > 51 ? 51 : want;
        }
    }
    pthread_mutex_unlock(&e->mu);
    return d;
}

static int dpb_find(Enc *e, int poc) { for (int i = 0; i < e->ndpb + 2 + 4; ++i) if (e->dpb_poc[i] == poc) return i; return -1; }   /* incl. the key pictures' and the anchor lane's own slots (unused ones hold no POC) */
static int dpb_free_slot(Enc *e, const int *keep, int nkeep)
{
    for (int i = 0; i < e->ndpb; ++i) {
        int k = 0;
        for (int q = 0; q < nkeep; ++q) if (e->dpb_poc[i] == keep[q]) k = 1;
        if (!k || e->dpb_poc[i] < 0) return i;
    }
    return -1;
}

/* ---- cuTree: the lookahead window's costs, propagation and finish (scheduler thread only; see Enc::ct_on) -------------------------------------------------------------------- */
static Input *input_at(Enc *e, int disp);
typedef struct CtNode { int b, p0, p1, is_ref; } CtNode;
/* the integer motion lambda of every QP (TEncParam+0x720 as recorded inside the reference: x264's table; the lookahead searches with entry 12 = 1, the others only matter where the
 * reference's cost table is overrun into its neighbouring rows) */
static const uint16_t kCtLambda[52] = {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 4, 4, 5, 5, 6, 7, 7, 8, 9, 11, 12, 13, 15, 17, 19, 21, 24, 27, 30, 34, 38, 42, 47, 53, 60, 67};
/* TEncParam words calcFrameCost reads, by preset (read inside the reference with every preset, -rc 3: zero_thr +0x3a0, fast_intra +0x3a4, +0x36c, +0x538, +0x3b4; +0x3a8 = 13 and
 * +0x8 = 0 throughout); blocks of 16 x 16 half-size samples from 1280 x 720 up and for ultrafast .. veryfast, else 8 x 8 */
static const struct { int zero_thr, fast_intra, f36c, f538, f3b4, lg4; } kCtPreset[9] = {{4, 4, 0, 120, 2, 1}, {4, 4, 0, 120, 2, 1}, {4, 1, 0, 0, 1, 1}, {0, 0, 1, 0, 1, 0}, {0, 0, 1, 0, 1, 0},
                                                                                              {0, 0, 1, 0, 1, 0}, {0, 0, 1, 0, 1, 0}, {0, 0, 1, 0, 1, 0}, {0, 0, 0, 0, 1, 0}};
static struct CtPic *ct_slot(Enc *e, int disp) { return &e->ct[((disp % CT_RING) + CT_RING) % CT_RING]; }
static int ct_open(Enc *e)                                             /* (the geometry - ct_w .. ct_stride - is lane_resolve's) */
{
    const size_t n = (size_t)e->ct_nx * e->ct_ny, lowsz = (size_t)e->ct_stride * (size_t)(e->ct_h + 2 * e->ct_pad);
    int r = ks265_create(&e->ctx_ct, e->dev_id);
    /* one block of device memory per picture of the ring: the padded half-size plane, then the per-block arrays (64-byte aligned) */
    const size_t a64 = 63;
    size_t off[16], o = (lowsz + a64) & ~a64;
    const size_t sz[14] = {n * 2, n * 2, n * 2, n * 2, n, (n + 3) / 4, n * 4, n * 4, n * 4, n * 4, n * 8, n * 8, sizeof(ks265_cfc_sums), 0};
    for (int k = 0; k < 13; ++k) { off[k] = o; o = (o + sz[k] + a64) & ~a64; }
    for (int i = 0; i < CT_RING && !r; ++i) {
        struct CtPic *c = &e->ct[i];
        c->disp = NO_PIC;
        r = ks265_dev_malloc(e->ctx_ct, (void **)&c->blk, o);
        if (r) break;
        c->low = c->blk + (size_t)e->ct_pad * e->ct_stride + e->ct_pad;
        c->intra = (uint16_t *)(c->blk + off[0]); c->invq = (uint16_t *)(c->blk + off[1]); c->prop = (uint16_t *)(c->blk + off[2]); c->inter = (uint16_t *)(c->blk + off[3]);
        c->imode = c->blk + off[4]; c->bits = c->blk + off[5]; c->mv0 = (int32_t *)(c->blk + off[6]); c->c0 = (int32_t *)(c->blk + off[7]); c->mv1 = (int32_t *)(c->blk + off[8]);
        c->c1 = (int32_t *)(c->blk + off[9]); c->aq_off = (double *)(c->blk + off[10]); c->qoff = (double *)(c->blk + off[11]); c->sums = (ks265_cfc_sums *)(c->blk + off[12]);
        r = ks265_event_create(e->ctx_ct, &c->ev_used);
    }
    if (!r) r = ks265_dev_malloc(e->ctx_ct, &e->ct_ws, ks265_calc_frame_cost_workspace(e->ct_nx, e->ct_ny));
    if (!r) r = ks265_dev_malloc(e->ctx_ct, (void **)&e->ct_acc, n * 16);
    if (!r) r = ks265_memset_async(e->ctx_ct, e->ct_acc, 0, n * 16);
    if (!r) r = ks265_dev_malloc(e->ctx_ct, (void **)&e->ct_scratch, 16);
    if (!r && e->aq_on) r = ks265_dev_malloc(e->ctx_ct, (void **)&e->ct_full, (size_t)e->W * e->H * 3 / 2);
    if (!r) r = ks265_event_create(e->ctx_ct, &e->ct_ev);
    return r;
}
static void ct_close(Enc *e)
{
    if (!e->ctx_ct) return;
    ks265_synchronize(e->ctx_ct);
    for (int i = 0; i < CT_RING; ++i) { ks265_dev_free(e->ctx_ct, e->ct[i].blk); if (e->ct[i].ev_used) ks265_event_destroy(e->ctx_ct, e->ct[i].ev_used); }
    ks265_dev_free(e->ctx_ct, e->ct_ws); ks265_dev_free(e->ctx_ct, e->ct_acc); ks265_dev_free(e->ctx_ct, e->ct_scratch); ks265_dev_free(e->ctx_ct, e->ct_full);
    if (e->ct_ev) ks265_event_destroy(e->ctx_ct, e->ct_ev);
    ks265_destroy(e->ctx_ct); e->ctx_ct = NULL;
}
/* picture `disp` in the ring: its half-size picture (downsample_c enc@0x4a6a60, edges replicated), its AQ offsets / inverse qscale factors (calcFrameAdaptQuant enc@0x4653c0 on the
 * lookahead's block grid, as the reference calls it; without -aq: zero offsets, factor 256) */
static int ct_prepare(Enc *e, int disp)
{
    struct CtPic *c = ct_slot(e, disp);
    if (c->disp == disp) return 0;
    Input *in = input_at(e, disp);
    if (!in) return KS265_FAIL;
    ks265_ctx *cx = e->ctx_ct;
    const int n = e->ct_nx * e->ct_ny;
    int r = c->used ? ks265_stream_wait_event(cx, c->ev_used) : 0;       /* the picture that held this slot CT_RING pictures ago: its QP map has been taken */
    c->disp = disp; c->p0 = c->p1 = NO_PIC; c->intra_done = 0;
    const uint8_t *full = NULL;
    if (in->dev) { if (!r && !in->up_sync) r = ks265_stream_wait_event(cx, in->ev_up); full = in->dev; }
    else if (e->ct_full) { if (!r) r = ks265_memcpy_h2d_async(cx, e->ct_full, in->i420, (size_t)e->W * e->H * 3 / 2); full = e->ct_full; }
    if (!r) r = full ? ks265_downsample_rect(cx, full, e->W, c->low, e->ct_stride, e->ct_w, e->ct_h) : ks265_downsample_from_host(cx, in->i420, e->W, c->low, e->ct_stride, e->ct_w, e->ct_h);
    if (!r) r = ks265_pad_plane(cx, c->low, e->ct_stride, e->ct_w, e->ct_h, e->ct_pad);
    if (!r && e->aq_on) r = ks265_frame_adapt_quant(cx, full, e->W, full + (size_t)e->W * e->H, full + (size_t)e->W * e->H * 5 / 4, e->W / 2, e->ct_nx, e->ct_ny, n, e->cfg.fAqStrength, c->aq_off, c->invq, e->ct_scratch);
    else if (!r) { r = ks265_memset_async(cx, c->aq_off, 0, (size_t)n * 8); if (!r) r = ks265_fill_u16(cx, c->invq, n, 256); }
    if (!r) r = ks265_memset_async(cx, c->sums, 0xff, sizeof(ks265_cfc_sums));      /* L+0x684 / +0x7c8 = -1: nothing computed yet */
    return r;
}
/* calcFrameCost of picture b against (p0, p1) (display indices; p1 < 0: none; p0 < 0: the intra pass alone), unless that is what its arrays hold */
static int ct_cost(Enc *e, int b, int p0, int p1)
{
    struct CtPic *c = ct_slot(e, b);
    if (p0 < 0) { if (c->intra_done) return 0; }
    else if (c->p0 == p0 && c->p1 == p1) return 0;
    const int ps = e->ct_preset;
    ks265_cfc_params q; memset(&q, 0, sizeof q);
    q.w = e->ct_w; q.h = e->ct_h; q.nx = e->ct_nx; q.ny = e->ct_ny; q.cnt = e->ct_nx * e->ct_ny; q.stride = e->ct_stride;
    q.d0 = p0 < 0 ? 0 : b - p0; q.d1 = p0 < 0 || p1 < 0 ? 0 : p1 - b; q.flag = 0; q.slice_type = p0 < 0 ? 2 : q.d1 ? 0 : 1;
    q.merange = 64; q.lg = e->ct_lg; q.zero_thr = kCtPreset[ps].zero_thr; q.fast_intra = kCtPreset[ps].fast_intra; q.scenecut = g_cli.scenecut ? g_cli.scenecut : 30; q.preset = ps; q.p8 = 0;
    q.aq = e->aq_on; q.b_intra = 1; q.f3a8 = 13; q.f36c = kCtPreset[ps].f36c; q.f538 = kCtPreset[ps].f538; q.f3b4 = kCtPreset[ps].f3b4;
    q.do_list[0] = q.d0 > 0; q.do_list[1] = q.d1 > 0; q.intra_done = c->intra_done;
    memcpy(q.lambda_tab, kCtLambda, sizeof q.lambda_tab);
    const int r = ks265_calc_frame_cost(e->ctx_ct, &q, c->low, q.d0 ? ct_slot(e, p0)->low : NULL, q.d1 ? ct_slot(e, p1)->low : NULL, c->intra, c->imode, c->invq, c->inter, c->bits,
                                        c->mv0, c->c0, c->mv1, c->c1, c->sums, e->ct_ws);
    if (p0 >= 0) { c->p0 = p0; c->p1 = p1; }
    if (q.d1 == 0) c->intra_done = 1;                                  /* (the reference marks the intra costs done after a pass without a list-1 picture only, enc@0x4a8be5) */
    return r;
}
/* the pictures of (lo, end] in coding order: mini-GOPs (lo, hi], (hi, hi + span], .. - the anchor P picture first, then its B pictures as the planner's walk gives them
 * (gop_walk).  The mini-GOPs behind the first are taken to be gop_b + 1 long: with the slice-type decision on as well that is a guess */
static int ct_structure(const Enc *e, int lo, int hi, int end, CtNode *out, int cap)
{
    int n = 0;
    const int span = e->gop_b + 1;
    while (lo < end && n < cap) {
        if (hi > end) hi = end;
        out[n++] = (CtNode){hi, lo, -1, 1};
        GopNode b[GOP_VIEW];
        const int nb = gop_walk(lo, hi, e->hier, b);
        for (int i = 0; i < nb && n < cap; ++i) out[n++] = (CtNode){b[i].b, b[i].lo, b[i].hi, b[i].is_ref};
        lo = hi; hi = lo + span;
    }
    return n;
}
/* the window's end for a mini-GOP that ends at display index a: ct_depth pictures further, inside this closed GOP, inside what has arrived.  -1: not all of it is there yet */
static int ct_window_end(Enc *e, int gop_start, int a, int iper, int have, int flush, int gop_end)
{
    int end = a + e->ct_depth;
    if (iper > 0 && end > gop_start + iper - 1) end = gop_start + iper - 1;
    if (gop_end >= a && end > gop_end) end = gop_end;
    for (int k = a + 1; k <= end && k < have; ++k) { const Input *ik = input_at(e, k); if (ik && ik->key) { end = k - 1; break; } }   /* a requested key picture closes the GOP in front of it */
    if (end >= have) { if (!flush) return -1; end = have - 1; }
    return end < a ? a : end;
}
/* costs + propagation over (first, end], then the offsets of the pictures in [fin_lo, fin_hi] (the key picture itself when key >= 0) */
static int ct_run(Enc *e, int key, int d, int a, int end)
{
    CtNode nodes[CT_RING];
    const int first = key >= 0 ? key : d;
    if (end - first >= CT_RING - 2) end = first + CT_RING - 3;
    const int nn = key >= 0 ? ct_structure(e, key, key + e->gop_b + 1, end, nodes, CT_RING) : ct_structure(e, d, a, end, nodes, CT_RING);
    const int n = e->ct_nx * e->ct_ny;
    int r = 0;
    for (int k = first; k <= end && !r; ++k) r = ct_prepare(e, k);
    for (int k = first; k <= end && !r; ++k) r = ks265_memset_async(e->ctx_ct, ct_slot(e, k)->prop, 0, (size_t)n * 2);       /* (the reference clears L+0x40 of the window before every pass, enc@0x480116) */
    if (!r && key >= 0) r = ct_cost(e, key, -1, -1);                  /* the key picture's intra costs (enc@0x480bb1) */
    for (int i = nn - 1; i >= 0 && !r; --i) {
        const CtNode *nd = &nodes[i];
        struct CtPic *c = ct_slot(e, nd->b), *r0 = ct_slot(e, nd->p0), *r1 = nd->p1 >= 0 ? ct_slot(e, nd->p1) : r0;
        r = ct_cost(e, nd->b, nd->p0, nd->p1);
        if (!r) r = ks265_cutree_propagate(e->ctx_ct, e->ct_lg, e->ct_nx, e->ct_ny, c->intra, c->invq, c->prop, c->inter, c->bits, c->mv0, nd->p1 >= 0 ? c->mv1 : c->mv0, r0->prop, r1->prop, e->ct_acc);
    }
    /* the finish for what is about to be coded: reference pictures get the tree's offsets, the others their AQ offsets alone (enc@0x480854..0x480a54) */
    for (int i = -1; i < nn && !r; ++i) {
        int b, is_ref, dbl = 0;
        if (i < 0) { if (key < 0) continue; b = key; is_ref = 1; }
        else { if (key >= 0 || nodes[i].b > a) continue; b = nodes[i].b; is_ref = nodes[i].is_ref; dbl = nodes[i].p1 < 0 && end == a; }   /* nothing of the window lies behind this mini-GOP: its anchor's
                                                                                                                                             * propagated cost counts twice (enc@0x480c6a, 0x4809d2) */
        struct CtPic *c = ct_slot(e, b);
        r = ks265_memcpy_d2d_async(e->ctx_ct, c->qoff, c->aq_off, (size_t)n * 8);
        if (!r && is_ref) r = ks265_cutree_finish(e->ctx_ct, n, c->intra, c->invq, c->prop, c->aq_off, dbl, c->qoff);
    }
    if (!r) r = ks265_event_record(e->ctx_ct, e->ct_ev);
    return r;
}

/* source against reconstruction: the SSE (-psnr), or with -ssim the fused pass that reads the two pictures once for both (the SSE sums bit for bit those of the SSE pass;
 * not wanted without -psnr).  on = NULL: the frame's own stream.  The SSIM sums then go home by a copy of their own on the same stream, in front of the picture's event */
static int quality_pass(Enc *e, ks265_ctx *on, ks265_frame *fr, ks265_pic src, ks265_pic rec, uint64_t *dsse, int64_t *dssim)
{
    if (dssim) return on ? ks265_ssim_picture_on(on, fr, src, rec, e->cfg.calcPsnr ? dsse : NULL, dssim) : ks265_ssim_picture(fr, src, rec, e->cfg.calcPsnr ? dsse : NULL, dssim);
    if (!e->cfg.calcPsnr) return 0;
    return on ? ks265_sse_picture_on(on, fr, src, rec, dsse) : ks265_sse_picture(fr, src, rec, dsse);
}

/* ---- submit(): one picture's GPU work + copies on the streams, then the hand-over to the writers - a sequence of steps (scheduler thread).  What the steps share travels in a
 *      Sub that submit() owns; nothing of it outlives the call.  Every device-library call of a step is skipped once an earlier one has failed (the lane is lost then: sched_err) */
typedef struct Sub {
    Job *j; Input *in;
    const GopPic *pic; int qp;                            /* what the planner decided about the picture (kind, POC, lists, keep set ..), and its QP */
    int k, recycled;                                      /* rotation slot of the input buffer / staging set (seq % NPIPE); it has held a picture before */
    int path; PixPath *p;                                 /* the pixel path that codes the picture (PATH_*) */
    int split, direct, graphable;
    int rslot;                                            /* `devrecon` / `analysis`: the pool slot the reconstruction and the analysis block are packed into (-1 without) */
    const int8_t *qmap;                                   /* the QP map set_qp_map handed to the frame object (NULL: the picture's QP everywhere) */
    const uint8_t *din; ks265_pic srcp; int slot; ks265_pic out;   /* the packed input on the device, the unpacked source picture, the reconstruction's DPB slot */
} Sub;

/* wait for a free job slot (the ring is full only if the consumer did not drain it: block on the oldest) */
static Job *wait_job_slot(Enc *e)
{
    pthread_mutex_lock(&e->mu);
    const double tw0 = now_ms();
    while (e->njobs == e->ring && !e->quit) {
        pthread_cond_broadcast(&e->cv_sched_done);                      /* a caller waiting for this thread in lane_put goes on and collects output instead */
        pthread_cond_wait(&e->cv_done, &e->mu);                         /* take_output signals when it has freed ring slots */
    }
    e->st.submit_wait_ms += now_ms() - tw0;
    Job *j = e->quit ? NULL : &e->jobs[e->job_tail];                    /* drained by take_output() of the calling thread itself: never full here */
    pthread_mutex_unlock(&e->mu);
    return j;
}

/* `devrecon`: a free slot of the pool, waited for like ring space (the calling thread's next call releases what its last one handed out); -1: the lane is closing */
static int wait_recon_slot(Enc *e)
{
    pthread_mutex_lock(&e->mu);
    const double tw0 = now_ms();
    int s;
    while ((s = recon_pool_take(&e->rpool)) < 0 && !e->quit) {
        pthread_cond_broadcast(&e->cv_sched_done);                      /* (as in wait_job_slot) */
        pthread_cond_wait(&e->cv_done, &e->mu);
    }
    e->st.submit_wait_ms += now_ms() - tw0;
    pthread_mutex_unlock(&e->mu);
    return s;
}

/* pixel path: the main stream / frame object, the key pictures' own or the anchors' own - the ONE place that decides it - and what follows from the choice */
static void choose_path(Enc *e, Sub *s)
{
    const int on_key = s->pic->kind == 'I' && e->key_overlap && (s->in->iper <= 0 || s->in->iper >= 32);
    const int on_anc = s->pic->kind == 'P' && !s->pic->gpb && e->anc_on && e->key_overlap && s->pic->nl0 == 1;      /* (key_overlap goes off with the reconstruction dump: everything on the main stream then) */
    s->path = on_key ? PATH_KEY : on_anc ? PATH_ANC : PATH_MAIN;
    s->p = &e->path[s->path];
    s->k = (int)(e->seq % NPIPE);
    s->recycled = e->seq >= NPIPE;
    s->split = e->split && s->path == PATH_MAIN;
    s->srcp = s->split ? e->srcq[s->k] : s->p->src;
    /* an anchor on its lane whose picture is on the device already waits for the upload itself: a mark on the copy-in stream would sit behind that stream's work for the
     * pictures in front of it - and, HIP streams sharing hardware queues (four by default), behind whatever else runs in that queue: measured, the anchor then starts when
     * the last B picture of the mini-GOP before it has left the device */
    s->direct = s->path == PATH_ANC && s->in->dev && !e->use_graph;
    /* graph path: a P picture with one reference on the main stream, once the first pictures have made every lazy allocation */
    s->graphable = e->use_graph && ((s->pic->kind == 'P' && s->pic->nl0 == 1 && !s->pic->gpb) || (s->pic->kind == 'B' && s->pic->nl0 == 1 && s->pic->nl1 == 1)) && s->path == PATH_MAIN && !e->recon_on && e->seq >= 8;
}

/* the input picture reaches the device and, unpacked and padded, the path's source picture */
static int stage_input(Enc *e, Sub *s)
{
    const size_t fsz = (size_t)e->W * e->H * 3 / 2;
    const int k = s->k; Input *in = s->in; ks265_ctx *cx = s->p->ctx;
    /* copy-in stream: the slot's previous picture must have been unpacked before the buffer is overwritten */
    int r = s->recycled ? ks265_stream_wait_event(e->ctx_in, e->ev_loaded[k]) : 0;
    if (!r && s->split && s->recycled) r = ks265_stream_wait_event(e->ctx_in, e->ev_drained[k]);   /* srcq[k]'s last reader (the SSE of three pictures ago) is through */
    /* with the lookahead the picture is on the device already, or on its way: uploaded into the slot's twin when it was handed in (round 4); else an H2D copy here, on this
     * stream, behind the waits above.  Graph replay needs fixed addresses: a device-to-device copy into the rotation buffer */
    s->din = e->dev_in[k];
    if (s->direct) { if (!r && !in->up_sync) r = ks265_stream_wait_event(cx, in->ev_up); s->din = in->dev; }     /* (see choose_path) */
    else if (in->dev) {
        if (!r && !in->up_sync) r = ks265_stream_wait_event(e->ctx_in, in->ev_up);
        if (!r && e->use_graph) r = ks265_memcpy_d2d_async(e->ctx_in, e->dev_in[k], in->dev, fsz);
        else s->din = in->dev;
    } else if (!r) r = ks265_memcpy_h2d_async(e->ctx_in, e->dev_in[k], in->i420, fsz);
    if (!r && s->split) r = ks265_load_i420_on(e->ctx_in, s->p->frame, s->din, s->srcp);
    if (!r && !s->direct) r = ks265_event_record(e->ctx_in, e->ev_h2d[k]);
    if (!r && !s->direct) r = ks265_stream_wait_event(cx, e->ev_h2d[k]);
    if (!s->graphable && !s->split) {
        if (!r) r = ks265_load_i420(s->p->frame, s->din, s->srcp);
        if (!r) r = ks265_event_record(cx, e->ev_loaded[k]);
    }
    return r;
}

/* the picture's QP and the tools it runs without */
static int set_picture_tools(Enc *e, Sub *s)
{
    ks265_frame *fr = s->p->frame;
    int r = ks265_frame_set_qp(fr, s->qp, s->pic->kind == 'I' ? kLambdaQ4[s->qp] : kLambdaInterQ4[s->qp]);
    /* the B pictures that run without intra candidates and SAO (lean 1), and without the joint refinement as well (lean 2): GopPic::lean */
    if (!r) r = s->pic->lean == 2 ? ks265_frame_set_picture_tools(fr, 0, 0, 0, e->lean_b == 2 && e->me_method == 2 ? 1 : -1) : s->pic->lean == 1 ? ks265_frame_set_picture_tools(fr, 0, -1, 0, -1) : ks265_frame_set_picture_tools(fr, -1, -1, -1, -1);
    /* `gpb`: the device runs the skip pass on every B slice (skip_rd 1 = B pictures only); an anchor is none to this host - its errors propagate through the pyramid */
    if (!r && e->gpb && ks265_frame_set_picture_skip) r = ks265_frame_set_picture_skip(fr, s->pic->gpb && e->fcfg.skip_rd < 2 ? 0 : -1);
    return r;
}

/* -rdoq 1: wait until every picture up to RC_LAG before this one is accounted (as the rate controller does), then the latest tables of this picture's kind among them */
static int set_rdoq_tables(Enc *e, Sub *s)
{
    if (!e->rdoq_on) return 0;
    if (s->pic->kind == 'I') { e->rq_gop_seq = e->rc_sub; return 0; }
    int32_t *tb = s->j->rq_host;
    pthread_mutex_lock(&e->mu);
    const long s0 = e->rc_sub, need = s0 - RC_LAG;
    for (;;) { rc_account(e); if (e->rc_acc_seq >= need || e->quit) break; pthread_cond_wait(&e->cv_done, &e->mu); }
    int found = 0;
    for (long q = need - 1; q >= 0 && q > e->rq_gop_seq && q >= need - (RQ_HIST - RC_LAG - 8) && !found; --q)
        if (e->rq_hist_kind[q % RQ_HIST] == (char)s->pic->kind) { memcpy(tb, e->rq_hist + (size_t)(q % RQ_HIST) * 1440, 1440 * sizeof(int32_t)); found = 1; }
    pthread_mutex_unlock(&e->mu);
    int r = 0;
    if (!found) r = ks265_rdoq_tables(&e->scfg, NULL, s->pic->kind == 'P' && !s->pic->gpb ? KS265_SLICE_P : KS265_SLICE_B, s->qp, tb) ? KS265_FAIL : 0;   /* (the slice type the picture goes out with) */
    memcpy(tb + 1440, e->rq_lam, sizeof e->rq_lam);
    if (!r) r = ks265_frame_set_rdoq(s->p->frame, tb, (const int64_t *)(tb + 1440), (const int64_t *)(tb + 1440) + 52);
    return r;
}

/* `roi`: one QP per CTU from the base offsets (the cuTree's, -aq's or none) and the picture's record (none: the base alone, bit for bit the plain entries) - in the base's
 * place, behind the same waits, + the wait for the record's filling (ks265_roi_reduce or the upload, on ctx_up) */
static int roi_ctu_map(Enc *e, Sub *s, ks265_ctx *ca, const double *base, int nx, int ny, int bpc, int lo, int hi, int8_t *qm)
{
    const Input *in = s->in;
    int r = in->roi_has ? ks265_stream_wait_event(ca, in->ev_roi) : 0;
    if (!r) r = ks265_roi_ctu_map(ca, in->roi_has ? in->roi_rec : NULL, base, nx, ny, bpc, e->geom.ctu_cols, e->geom.ctu_rows, s->qp, lo, hi, qm);
    return r;
}

/* one QP per CTU around this picture's QP (cuTree, else -aq; `roi`: + the caller's offsets): the map is made, handed to the frame object and copied home for the writer */
static int set_qp_map(Enc *e, Sub *s)
{
    if (!e->qmap_on) return 0;
    const int k = s->k; PixPath *p = s->p;
    ks265_ctx *ca = s->split ? e->ctx_in : p->ctx;
    /* a key picture on its own stream runs beside the pictures of earlier GOPs - among them the one three submissions back, whose kernels still read dev_qmap[k]
     * (ADVICE r4): it gets a map of its own; everything that touches that one is on the key pictures' stream, in order */
    int8_t *qm = s->path == PATH_KEY ? e->dev_qmap_key[e->nkeys & 1] : e->dev_qmap[k];
    int r = 0;
    if (e->ct_on) {
        /* cuTree: the picture's block offsets were finished on the lookahead's stream when its mini-GOP was scheduled (ct_run): one QP per CTU around this picture's QP */
        struct CtPic *cp = ct_slot(e, s->in->disp);
        if (cp->disp != s->in->disp) r = KS265_FAIL;
        if (!r) r = ks265_stream_wait_event(ca, e->ct_ev);
        if (!r && e->roi_on) r = roi_ctu_map(e, s, ca, cp->qoff, e->ct_nx, e->ct_ny, 64 >> (e->ct_lg + 1), e->cfg.qpmin, e->cfg.qpmax ? e->cfg.qpmax : 51, qm);
        else if (!r) r = ks265_qoff_ctu_map(ca, cp->qoff, e->ct_nx, e->ct_ny, e->ct_lg, e->geom.ctu_cols, e->geom.ctu_rows, s->qp, e->cfg.qpmin, e->cfg.qpmax ? e->cfg.qpmax : 51, qm);
        if (!r) r = ks265_event_record(ca, cp->ev_used);
        cp->used = 1;
    } else if (e->aq_on) {
        /* the source picture is on the device: block variances -> offsets (the reference's arithmetic) -> one QP per CTU around this picture's QP.  With the split pipeline
         * this runs on the copy-in stream right behind the unpack (off the pixel path's chain: the mean is a sequential sum, 0.15 ms at 2160p); the map stays in its rotation
         * slot while the picture's kernels and the copy-home run */
        const size_t oy = (size_t)e->geom.pad_y * e->geom.stride_y + e->geom.pad_y, oc = (size_t)e->geom.pad_c * e->geom.stride_c + e->geom.pad_c;
        r = ks265_frame_adapt_quant(ca, s->srcp.y + oy, e->geom.stride_y, s->srcp.u + oc, s->srcp.v + oc, e->geom.stride_c, e->aq_nx, e->aq_ny, e->aq_nx * e->aq_ny, e->cfg.fAqStrength,
                                    p->aq_off, p->aq_inv, p->aq_scratch);
        if (!r && e->roi_on) r = roi_ctu_map(e, s, ca, p->aq_off, e->aq_nx, e->aq_ny, 4, e->cfg.rc ? e->cfg.qpmin : 0, e->cfg.rc && e->cfg.qpmax ? e->cfg.qpmax : 51, qm);
        else if (!r) r = ks265_aq_ctu_map(ca, p->aq_off, e->aq_nx, e->aq_ny, s->qp, e->cfg.rc ? e->cfg.qpmin : 0, e->cfg.rc && e->cfg.qpmax ? e->cfg.qpmax : 51, qm);
    } else r = roi_ctu_map(e, s, ca, NULL, 0, 0, 4, e->cfg.rc ? e->cfg.qpmin : 0, e->cfg.rc && e->cfg.qpmax ? e->cfg.qpmax : 51, qm);   /* `roi` alone: the picture's QP + the caller's offsets (-aq's bounds) */
    if (!r) r = ks265_frame_set_qp_map(p->frame, qm);
    s->qmap = qm;
    if (!r) r = ks265_memcpy_d2h_async(ca, s->j->qp_map, qm, (size_t)e->geom.ctu_cols * e->geom.ctu_rows);
    if (!r && s->split) { r = ks265_event_record(e->ctx_in, e->ev_h2d[k]); if (!r) r = ks265_stream_wait_event(p->ctx, e->ev_h2d[k]); }   /* (recorded again behind the map: the pixel path waits for this one) */
    return r;
}

/* where the reconstruction goes: a free DPB slot, or one of the rotating slots the key pictures and the anchors own - those once their previous readers are through */
static int choose_recon_slot(Enc *e, Sub *s)
{
    ks265_ctx *cx = s->p->ctx;
    int r = 0;
    switch (s->path) {
    case PATH_KEY:
        s->slot = e->ndpb + (e->nkeys & 1);
        /* everything enqueued on the main stream so far belongs to earlier GOPs: when this mark fires, the readers of the previous key picture are through.
         * The slot written now held the key picture two GOPs back: wait for the mark set when the previous key picture was submitted */
        if (e->nkeys >= 1) r = ks265_event_record(main_ctx(e), e->ev_firstp[(e->nkeys - 1) & 1]);
        if (!r && e->nkeys >= 2) r = ks265_stream_wait_event(cx, e->ev_firstp[e->nkeys & 1]);
        break;
    case PATH_ANC:
        s->slot = e->ndpb + 2 + (e->nanch & 3);
        /* the slot held the anchor four back, which closed mini-GOP nanch - 4; its readers on the main stream were the B pictures of mini-GOPs nanch - 4 and nanch - 3 */
        if (e->nanch >= 4) r = ks265_stream_wait_event(cx, e->ev_mg[(e->nanch - 3) & 7]);
        break;
    default:
        s->slot = dpb_free_slot(e, s->pic->keep, s->pic->nk);
    }
    if (s->slot < 0) return KS265_FAIL;
    s->out = e->dpb[s->slot];
    return r;
}

/* the picture's kernels: THE dispatch onto the device library's four entries - key picture / P / P with several references / B / B with several references per list */
static int code_picture(Enc *e, const Sub *s)
{
    ks265_frame *fr = s->p->frame;
    ks265_pic r0[4], r1[4];
    for (int i = 0; i < s->pic->nl0; ++i) r0[i] = e->dpb[dpb_find(e, s->pic->l0[i])];
    for (int i = 0; i < s->pic->nl1; ++i) r1[i] = e->dpb[dpb_find(e, s->pic->l1[i])];
    if (s->pic->kind == 'B' || s->pic->gpb) return s->pic->nl0 > 1 || s->pic->nl1 > 1 ? ks265_encode_picture_b_mref(fr, s->srcp, r0, s->pic->nl0, r1, s->pic->nl1, s->out) : ks265_encode_picture_b(fr, s->srcp, r0[0], r1[0], s->out);
    if (s->pic->kind == 'P' && s->pic->nl0 > 1) return ks265_encode_picture_mref(fr, s->srcp, r0, s->pic->nl0, s->out);
    const int key = s->pic->kind == 'I';
    return ks265_encode_picture(fr, s->srcp, key ? s->out : r0[0], key, s->out);
}

/* the reconstruction comes back to the host (reconstruction dump / -md5): on the picture's own stream */
static int recon_home(Enc *e, const Sub *s)
{
    int r = ks265_store_i420(s->p->frame, s->out, e->dev_recon);
    if (!r) r = ks265_memcpy_d2h_async(s->p->ctx, s->j->recon, e->dev_recon, (size_t)e->W * e->H * 3 / 2);
    return r;
}

/* `devrecon`: the output picture packed into the picture's own pool slot, on the picture's own stream - behind the last conversion that read the slot's previous picture */
static int recon_pack(Enc *e, const Sub *s)
{
    struct ReconSlot *q = &e->rslot[s->rslot];
    int r = q->read_on ? ks265_stream_wait_event(s->p->ctx, q->ev_read) : 0;
    if (!r) r = ks265_store_i420(s->p->frame, s->out, q->dev);
    return r;
}

/* `analysis`: the picture's CU map, QP map and block error packed into the slot's analysis block, on the picture's own stream - behind the last export that read the block.  The
 * reference indices of the CU map are resolved here: delta[L][i] = POC of list L's picture i - the picture's POC */
static int analysis_pack(Enc *e, const Sub *s)
{
    struct ReconSlot *q = &e->rslot[s->rslot];
    int8_t delta[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
    for (int i = 0; i < s->pic->nl0 && i < 4; ++i) { const int d = s->pic->l0[i] - s->pic->poc; delta[0][i] = (int8_t)(d < -128 ? -128 : d > 127 ? 127 : d); }
    for (int i = 0; i < s->pic->nl1 && i < 4; ++i) { const int d = s->pic->l1[i] - s->pic->poc; delta[1][i] = (int8_t)(d < -128 ? -128 : d > 127 ? 127 : d); }
    int r = q->read_on_an ? ks265_stream_wait_event(s->p->ctx, q->ev_read_an) : 0;
    if (!r) r = ks265_analysis_pack(s->p->frame, s->srcp, s->out, NULL, s->qmap, s->qp, delta, q->an);
    return r;
}

/* what a picture leaves in its pool slot (pool_on), and ONE record of the slot's ev_packed behind the last of it */
static int slot_packs(Enc *e, const Sub *s)
{
    int r = e->devrecon ? recon_pack(e, s) : 0;
    if (!r && e->analysis) r = analysis_pack(e, s);
    if (!r) r = ks265_event_record(s->p->ctx, e->rslot[s->rslot].ev_packed);
    return r;
}

/* the drain of a coded picture: quality pass, its SSIM sums home, the records packed into the staging set of the rotation slot.  on = NULL: on the picture's own stream - there
 * the reconstruction goes home in between, and the staging block must have been copied out before it is written.  captured: inside a graph capture (or its launch-by-launch
 * repeat) - the pass and the packing alone; the wait is in front of the capture, the SSIM copy behind it (not part of the captured picture: every job has its own buffer) */
static int drain_picture(Enc *e, const Sub *s, ks265_ctx *on, int captured)
{
    const PixPath *p = s->p;
    ks265_ctx *cx = on ? on : p->ctx;
    const void *extra = e->cfg.calcPsnr ? p->dev_sse : NULL;
    int r = quality_pass(e, on, p->frame, s->srcp, s->out, p->dev_sse, p->dev_ssim);
    if (!r && e->ragged && e->cfg.calcPsnr) r = ks265_sse_window(cx, p->frame, s->srcp, s->out, e->srcW, e->srcH, p->dev_sse);   /* behind the pass, on its stream: the window's sums */
    if (!r && p->dev_ssim && !captured) r = ks265_memcpy_d2h_async(cx, s->j->ssim, p->dev_ssim, 24);
    /* `hash`: CRC and checksum of the output picture (one read of it), home the same way */
    if (!r && p->dev_hash) r = on ? ks265_picture_hash_on(on, p->frame, s->out, p->dev_hash) : ks265_picture_hash(p->frame, s->out, p->dev_hash);
    if (!r && p->dev_hash && !captured) r = ks265_memcpy_d2h_async(cx, s->j->hash, p->dev_hash, 24);
    if (!on && !captured) {
        if (!r && e->recon_on) r = recon_home(e, s);
        if (!r && e->pool_on) r = slot_packs(e, s);
        /* the records leave the frame object's buffers for a staging set (device to device, a few microseconds), so that the next picture can start
         * while the copy-out stream drains this one */
        if (!r && s->recycled) r = ks265_stream_wait_event(cx, e->ev_drained[s->k]);
    }
    if (!r) r = on ? ks265_frame_pack_compact_on(on, p->frame, e->stg[s->k], extra) : ks265_frame_pack_compact(p->frame, e->stg[s->k], extra);
    return r;
}

/* what a graph holds: the launches of one picture on the main stream - unpack, kernels, drain */
static int picture_launches(Enc *e, const Sub *s)
{
    int r = ks265_load_i420(s->p->frame, e->dev_in[s->k], s->srcp);
    if (!r) r = code_picture(e, s);
    if (!r) r = drain_picture(e, s, NULL, 1);
    return r;
}

/* single-reference P and B pictures on the main stream as graphs (Enc::use_graph): replay of the captured picture, or its capture */
static int code_picture_graph(Enc *e, Sub *s)
{
    const int k = s->k; PixPath *p = s->p; ks265_ctx *cx = p->ctx; ks265_frame *fr = p->frame;
    const ks265_pic refp = e->dpb[dpb_find(e, s->pic->l0[0])], ref1p = s->pic->kind == 'B' ? e->dpb[dpb_find(e, s->pic->l1[0])] : refp;
    const uint64_t key[9] = {(uint64_t)(uintptr_t)refp.y, (uint64_t)(uintptr_t)s->out.y, (uint64_t)(uintptr_t)e->dev_in[k], (uint64_t)(uintptr_t)e->stg[k],
                             (uint64_t)s->qp, (uint64_t)ks265_frame_p_state(fr), (uint64_t)(e->cfg.calcPsnr != 0) | (uint64_t)e->ssim_on << 1 | (uint64_t)(e->hash_on != 0) << 2, (uint64_t)s->pic->kind | ((uint64_t)s->pic->lean << 8), (uint64_t)(uintptr_t)ref1p.y};
    void *exec = NULL;
    for (int i = 0; i < e->ngraph && !exec; ++i) if (!memcmp(e->graph[i].key, key, sizeof key)) exec = e->graph[i].exec;
    int r = s->recycled ? ks265_stream_wait_event(cx, e->ev_drained[k]) : 0;       /* the staging block of this rotation slot has been copied out */
    if (!r && exec) {
        r = ks265_graph_launch(cx, exec);
        if (!r && s->pic->kind == 'P') r = ks265_frame_p_advance(fr);              /* a B picture leaves the P pictures' predictor chain alone */
    } else if (!r) {
        int keep_it = e->ngraph < MAX_GRAPHS;
        const int state0 = ks265_frame_p_state(fr);
        if (keep_it && ks265_capture_begin(cx)) { keep_it = 0; e->use_graph = 0; }   /* no capture on this runtime: launch by launch from here on */
        r = picture_launches(e, s);
        if (keep_it) {
            void *ex = NULL;
            const int rc = ks265_capture_end(cx, &ex);                      /* also ends a capture that failed half-way */
            if (!r && !rc) { memcpy(e->graph[e->ngraph].key, key, sizeof key); e->graph[e->ngraph].exec = ex; ++e->ngraph; r = ks265_graph_launch(cx, ex); }
            else if (!r) {                                                  /* recorded but not instantiated: nothing ran.  Do the picture launch by launch, graphs off */
                e->use_graph = 0;
                r = ks265_frame_p_restore(fr, state0);
                if (!r) r = picture_launches(e, s);
            }
        }
    }
    if (!r && p->dev_ssim) r = ks265_memcpy_d2h_async(cx, s->j->ssim, p->dev_ssim, 24);  /* (see drain_picture) */
    if (!r && p->dev_hash) r = ks265_memcpy_d2h_async(cx, s->j->hash, p->dev_hash, 24);
    if (!r) r = ks265_event_record(cx, e->ev_loaded[k]);                  /* the input buffer is free again (a little later than on the plain path) */
    if (!r) r = ks265_event_record(cx, e->ev_staged[k]);
    e->dpb_poc[s->slot] = s->pic->poc;
    return r;
}

/* launch by launch: the kernels on the path's stream; the drain behind them there, or - split pipeline - on the copy-out stream */
static int code_picture_plain(Enc *e, Sub *s)
{
    const int k = s->k; PixPath *p = s->p; ks265_ctx *cx = p->ctx;
    int r = code_picture(e, s);
    if (!r && s->pic->kind == 'I' && s->path == PATH_MAIN) r = ks265_frame_p_restore(p->frame, 0);   /* (a key picture on the main stream: see mark_streams) */
    e->dpb_poc[s->slot] = s->pic->poc;
    if (!s->split) {
        if (!r) r = drain_picture(e, s, NULL, 0);
        if (!r) r = ks265_event_record(cx, e->ev_staged[k]);
        return r;
    }
    if (!r && e->recon_on) r = recon_home(e, s);
    if (!r && e->pool_on) r = slot_packs(e, s);                         /* (the split pipeline's drain_picture runs on the copy-out stream: the packs stay on the picture's own) */
    /* the drain runs on the copy-out stream (in order with the earlier pictures' drains: the staging block of this slot has been copied out before it is written) */
    if (!r) r = ks265_event_record(cx, e->ev_coded[k]);
    if (!r) r = ks265_stream_wait_event(e->ctx_out, e->ev_coded[k]);
    if (!r) r = drain_picture(e, s, e->ctx_out, 0);
    if (!r) r = ks265_event_record(e->ctx_out, e->ev_packed[k]);
    if (!r) r = ks265_event_record(e->ctx_out, e->ev_staged[k]);
    if (!r) r = ks265_frame_set_records_fence(p->frame, e->ev_packed[k]);   /* the next picture on this frame object: its search starts now, its first record waits */
    return r;
}

/* the cross-stream marks behind a key picture or an anchor: who waits for it, whose temporal predictors start over */
static int mark_streams(Enc *e, Sub *s)
{
    ks265_ctx *cx = s->p->ctx;
    PixPath *anc = &e->path[PATH_ANC];
    int r = 0;
    if (s->path == PATH_KEY) {                                         /* everything coded after it on the main stream waits for the key picture; its temporal predictors start over */
        if (!r) r = ks265_event_record(cx, e->ev_key);
        if (!r) r = ks265_stream_wait_event(main_ctx(e), e->ev_key);
        if (!r) r = ks265_frame_p_restore(main_frame(e), 0);            /* temporal predictors start over, and so does the ping-pong of the PU record buffers: the graph keys of a GOP's
                                                                         * pictures (which hold that state) are the same in every GOP - nothing is captured after the first one */
        if (!r && e->anc_on) { r = ks265_stream_wait_event(anc->ctx, e->ev_key); if (!r) r = ks265_frame_p_restore(anc->frame, 0); }   /* the first anchor predicts from it */
        ++e->nkeys;
    }
    if (s->pic->kind == 'I' && s->path == PATH_MAIN && e->anc_on) {         /* a key picture on the main stream (short intra period): the anchors' stream waits for it there */
        if (!r) r = ks265_event_record(main_ctx(e), e->ev_key);
        if (!r) r = ks265_stream_wait_event(anc->ctx, e->ev_key);
        if (!r) r = ks265_frame_p_restore(anc->frame, 0);
    }
    e->last_on_anc = s->path == PATH_ANC;
    if (s->path == PATH_ANC) {                                         /* the B pictures in front of it (and everything else the main stream codes from here on) wait for the anchor */
        if (!r) r = ks265_event_record(cx, e->ev_anc);
        if (!r) r = ks265_stream_wait_event(main_ctx(e), e->ev_anc);
        ++e->nanch;
    }
    return r;
}

/* copy-out stream: the staged records go home, then the picture's event */
static int copy_out(Enc *e, const Sub *s)
{
    const int k = s->k;
    int r = ks265_stream_wait_event(e->ctx_out, e->ev_staged[k]);
    /* the records go home: the fixed part + the stored lines only (~2 MB for a P picture at 2160p), by a kernel that reads the size on the device (or, KS265_COPYOUT_MB,
     * a fixed amount by hipMemcpyAsync and the rest by that kernel) */
    if (!r) r = e->copy_mb < 0 ? ks265_copy_out_compact_async(e->ctx_out, main_frame(e), s->j->cmp, e->stg[k])
                               : ks265_copy_out_compact_dma_async(e->ctx_out, main_frame(e), s->j->cmp, e->stg[k], s->pic->kind == 'I' ? e->cmp_off[7] : (size_t)e->copy_mb << 20);
    if (!r) r = ks265_event_record(e->ctx_out, e->ev_drained[k]);
    if (!r) r = ks265_event_record(e->ctx_out, s->j->ev);
    return r;
}

/* what the writer needs to know about the picture */
static void fill_job(Enc *e, const Sub *s)
{
    Job *j = s->j; const Input *in = s->in;
    j->no_sao = s->pic->lean != 0;
    j->rslot = s->rslot;
    j->disp = in->disp; j->pts = in->pts; j->poc = s->pic->poc; j->kind = s->pic->kind; j->qp = s->qp; j->is_ref = s->pic->is_ref; j->key_headers = s->pic->key_headers; j->rc_delta = e->rc_qp_delta;
    j->rc_budget = (double)in->kbps * 1000.0 / (e->cfg.frameRate > 0 ? e->cfg.frameRate : 25.0);
    j->nal_type = s->pic->kind == 'I' ? KS265_NAL_IDR_W_RADL : s->pic->is_ref ? KS265_NAL_TRAIL_R : KS265_NAL_TRAIL_N;
    j->gpb = s->pic->gpb;
    j->nl0 = s->pic->nl0; j->nl1 = s->pic->nl1;
    for (int i = 0; i < s->pic->nl0; ++i) j->l0[i] = s->pic->l0[i];
    for (int i = 0; i < s->pic->nl1; ++i) j->l1[i] = s->pic->l1[i];
    /* RPS: the picture's keep set - what must stay for later pictures + what this picture uses */
    j->nrps = 0;
    if (s->pic->kind != 'I')
        for (int i = 0; i < s->pic->nk; ++i) {
            int dup = 0;
            for (int q = 0; q < j->nrps; ++q) if (j->rps_poc[q] == s->pic->keep[i]) dup = 1;
            if (dup || s->pic->keep[i] == s->pic->poc) continue;
            int used = 0;
            for (int q = 0; q < s->pic->nl0; ++q) if (s->pic->l0[q] == s->pic->keep[i]) used = 1;
            for (int q = 0; q < s->pic->nl1; ++q) if (s->pic->l1[q] == s->pic->keep[i]) used = 1;
            j->rps_poc[j->nrps] = s->pic->keep[i]; j->rps_used[j->nrps++] = (unsigned char)used;
        }
    j->t_submit = now_ms();
}

/* the job joins the ring: the dispatcher waits for its event, the writers take it from there */
static void publish_job(Enc *e, const Sub *s)
{
    Job *j = s->j;
    pthread_mutex_lock(&e->mu);
    s->in->used = IN_CODING;                                           /* under the lock: the caller counts the pictures in flight */
    j->done = 0; j->error = 0; j->used = 1; j->started = 0; j->nrows = 0; j->next_row = 0; j->rows_done = 0; j->sei_len = 0;
    j->sub_seq = e->rc_sub;
    e->job_tail = (e->job_tail + 1) % e->ring; ++e->njobs; ++e->nwait; ++e->rc_sub;
    e->st.occ_samples++; e->st.occ_ring += e->njobs; e->st.occ_gpu += e->nwait; e->st.occ_ready += e->npending;
    pthread_cond_signal(&e->cv_disp);
    pthread_cond_broadcast(&e->cv_sched_done);                         /* progress: a caller waiting for the scheduler (input back-pressure, flush) looks again */
    pthread_mutex_unlock(&e->mu);
}

/* enqueue one picture: GPU work + copies on the streams, then hand it to the writers */
static int submit(Enc *e, Input *in, const GopPic *pic, int qp)
{
    Sub s = {.in = in, .pic = pic, .qp = qp};
    if (!(s.j = wait_job_slot(e))) return QY_FAIL;
    s.rslot = -1;
    if (e->pool_on && (s.rslot = wait_recon_slot(e)) < 0) return QY_FAIL;
    choose_path(e, &s);
    int r = stage_input(e, &s);
    if (!r) r = set_picture_tools(e, &s);
    if (!r) r = set_rdoq_tables(e, &s);
    if (!r) r = set_qp_map(e, &s);
    if (!r) r = choose_recon_slot(e, &s);
    if (!r) r = s.graphable ? code_picture_graph(e, &s) : code_picture_plain(e, &s);
    if (!r) r = mark_streams(e, &s);
    if (!r) r = copy_out(e, &s);
    if (r) {
        if (s.rslot >= 0) { pthread_mutex_lock(&e->mu); (void)recon_pool_untake(&e->rpool, s.rslot); pthread_mutex_unlock(&e->mu); }
        return hip_rc(r);
    }
    ++e->seq;
    fill_job(e, &s);
    publish_job(e, &s);
    return QY_OK;
}

/* the input slot of display index disp (scheduler thread; under the lock: the caller's thread marks slots while it fills them) */
static Input *input_at(Enc *e, int disp)
{
    Input *r = NULL;
    pthread_mutex_lock(&e->mu);
    for (int i = 0; i < MAX_INPUT && !r; ++i) if (e->in[i].used == IN_READY && e->in[i].disp == disp) r = &e->in[i];
    pthread_mutex_unlock(&e->mu);
    return r;
}
static int clampqp(Enc *e, int q) { int lo = e->cfg.rc ? e->cfg.qpmin : 0, hi = e->cfg.rc ? (e->cfg.qpmax ? e->cfg.qpmax : 51) : 51; return q < lo ? lo : q > hi ? hi : q; }

/* what the planner may ask about the pictures behind display index d, and their slots for the executor: one lock, one pass over the table */
static void gather_view(Enc *e, int d, int flush, int have, int gop_end, GopView *v, Input *slot[GOP_VIEW])
{
    memset(v, 0, sizeof *v); memset(slot, 0, GOP_VIEW * sizeof *slot);
    v->have = have; v->flush = flush; v->gop_end = gop_end;
    pthread_mutex_lock(&e->mu);
    for (int i = 0; i < MAX_INPUT; ++i) {
        Input *in = &e->in[i];
        const int k = in->disp - (d + 1);
        if (in->used != IN_READY || k < 0 || k >= GOP_VIEW || slot[k]) continue;
        slot[k] = in; v->at[k].present = 1; v->at[k].key = in->key; v->at[k].mini4 = in->mini4; v->at[k].iper = in->iper;
    }
    pthread_mutex_unlock(&e->mu);
}

/* schedule whatever can be coded with the pictures received so far; flush = no more input will come.  View -> plan -> execute: every GOP decision is gop_plan's (ks265_gop.h);
 * this loop waits, asks the rate controller and enqueues.  Nothing of a unit has happened before it is certain to be submitted: the plan is made on a copy of the state */
static int schedule(Enc *e, int flush, int have /* pictures [0, have) have arrived */, int gop_end /* a GOP ends at this picture whatever follows, or -1 */)
{
    for (;;) {
        const int d = e->coded_upto;                                   /* last anchor / last coded display index; -1 before the first picture */
        GopView v; Input *slot[GOP_VIEW]; GopUnit u;
        GopState st = e->gs;
        gather_view(e, d, flush, have, gop_end, &v, slot);
        const int what = gop_plan(&e->rules, &st, &v, d, &u);
        if (what != GOP_UNIT) return what == GOP_WAIT ? QY_OK : QY_FAIL;   /* (gone: an error elsewhere emptied the input table under the scheduler) */
        if (e->ct_on) {                                                /* cuTree: costs and propagation over the window behind this key picture / mini-GOP, offsets for its pictures */
            const int end = ct_window_end(e, st.gop_start, u.a, u.iper, have, flush, gop_end);
            if (end < 0) return QY_OK;
            const int rr = u.key ? ct_run(e, u.a, u.a, u.a, end) : ct_run(e, -1, d, u.a, end);
            if (rr) return hip_rc(rr);
        }
        e->gs = st;
        e->rc_qp_delta = rc_decide(e);                                 /* rate control: one offset per key picture / mini-GOP, decided when it is certain to be submitted */
        if (u.key) for (int i = 0; i < e->ndpb + 2 + 4; ++i) e->dpb_poc[i] = NO_PIC;
        int anchor_on_lane = 0;
        for (int i = 0; i < u.n; ++i) {
            const GopPic *p = &u.pic[i];
            Input *in = slot[p->disp - (d + 1)];                       /* (looked up once per unit: a tear-down that empties the table while the unit is submitted is noticed at the next unit, or by submit itself - wait_job_slot) */
            const int r = submit(e, in, p, clampqp(e, in->base_qp + e->rc_qp_delta + p->qp_off));
            if (r) return r;
            if (i == 0) anchor_on_lane = e->last_on_anc;
        }
        if (!u.key && e->anc_on && anchor_on_lane) {   /* every B picture that reads the anchors of this mini-GOP is on the main stream now */
            const int r = hip_rc(ks265_event_record(main_ctx(e), e->ev_mg[(e->nanch - 1) & 7]));
            if (r) return r;
        }
        pthread_mutex_lock(&e->mu); e->coded_upto = u.a; pthread_mutex_unlock(&e->mu);
    }
}

/* ---- the scheduler thread: runs schedule() whenever pictures have arrived (or a flush was asked for).  The caller's thread only copies the input
 *      picture and collects output; this thread takes the GOP decisions and enqueues the GPU work of every picture. */
static int la_drain(Enc *e, int keep);
static void reg_handle(ks265_ctx *c, int open);
static void *scheduler(void *arg)
{
    Enc *e = (Enc *)arg;
    pthread_mutex_lock(&e->mu);
    for (;;) {
        while (!e->quit && e->sched_seen == e->next_disp && !e->sched_flush && e->gop_end_seen == e->gop_end) {
            e->sched_idle = 1; pthread_cond_broadcast(&e->cv_sched_done);
            if (e->la_on && __atomic_load_n(&e->la_qn, __ATOMIC_ACQUIRE) > 0) {
                /* pictures sit at the input until their lookahead results have arrived, and the caller only looks when it hands in the next picture - it may be asleep (its
                 * back-pressure, the output ring): with nothing to schedule this thread looks as well */
                struct timespec ts; clock_gettime(CLOCK_REALTIME, &ts);
                ts.tv_nsec += 200000; if (ts.tv_nsec >= 1000000000) { ts.tv_nsec -= 1000000000; ++ts.tv_sec; }
                pthread_cond_timedwait(&e->cv_sched, &e->mu, &ts);
                if (e->quit || e->sched_seen != e->next_disp || e->sched_flush) continue;
                pthread_mutex_unlock(&e->mu);
                (void)la_drain(e, LA_QMAX);                             /* (never waits: the queue's size) */
                pthread_mutex_lock(&e->mu);
                if (e->sched_seen != e->next_disp) ++e->la_n_poll;
            } else pthread_cond_wait(&e->cv_sched, &e->mu);
        }
        if (e->quit) break;
        e->sched_idle = 0;
        const int flush = e->sched_flush, have = e->next_disp, gop_end = e->gop_end;
        pthread_mutex_unlock(&e->mu);
        const double t0 = now_ms();
        const int r = schedule(e, flush, have, gop_end);
        const double dt = now_ms() - t0;
        pthread_mutex_lock(&e->mu);
        e->st.submit_ms += dt;
        if (r && !e->sched_err) e->sched_err = r;
        e->sched_seen = have; e->gop_end_seen = gop_end;
        if (flush && have == e->next_disp) e->sched_flush = 0;          /* everything that had arrived is scheduled */
    }
    e->sched_idle = 1;
    pthread_cond_broadcast(&e->cv_sched_done);
    pthread_mutex_unlock(&e->mu);
    return NULL;
}

/* move finished pictures (in coding order) to the output array; wait while more than `max_in_flight` pictures are queued
 * (0 = drain everything, MAX_JOBS = never wait) */
static int take_output(Enc *e, int max_in_flight, int max_pics, QY265Nal **pNals, int *n, QY265Picture *out, int *pics)
{
    int cnt = 0, err = QY_OK, taken = 0;
    e->outpos = 0;
    pthread_mutex_lock(&e->mu);
    while (e->njobs && taken < max_pics) {
        Job *j = &e->jobs[e->job_head];
        if (!j->done) { if (e->njobs <= max_in_flight) break; pthread_cond_wait(&e->cv_done, &e->mu); continue; }
        if (j->error) err = hip_rc(j->error);
        const size_t nsl = (size_t)(j->nal_len > 0 ? j->nal_len : 0), nsei = (size_t)(j->nal_len > 0 && j->sei_len > 0 ? j->sei_len : 0), need = nsl + nsei;
        if (e->outpos + need > e->outcap) {                             /* the caller reads the payloads after this call: they cannot stay in the job (its slot is reused) */
            if (cnt) break;                                             /* hand out what fits, the rest next time */
            uint8_t *nb = (uint8_t *)realloc(e->outbuf, need + 65536);
            if (!nb) { err = QY_OUTOFMEMORY; break; }
            e->outbuf = nb; e->outcap = need + 65536;
        }
        if (j->key_headers && e->cfg.bHeaderBeforeKeyframe) {
            long off = 0;                                               /* the three parameter sets as separate NAL entries */
            for (int k = 0; k < 3; ++k) {
                e->nals[cnt].naltype = KS265_NAL_VPS + k; e->nals[cnt].tid = 0; e->nals[cnt].iSize = (int)e->hdr_part[k]; e->nals[cnt].pts = j->pts; e->nals[cnt].pPayload = e->hdr + off;
                ++cnt; off += e->hdr_part[k];
            }
        }
        memcpy(e->outbuf + e->outpos, j->nal, nsl);
        e->nals[cnt].naltype = j->nal_type; e->nals[cnt].tid = 0; e->nals[cnt].iSize = (int)nsl; e->nals[cnt].pts = j->pts; e->nals[cnt].pPayload = e->outbuf + e->outpos;
        e->outpos += nsl;
        ++cnt;
        if (nsei) {                                                     /* `hash`: the picture's SEI message, one more NAL unit with the picture's pts */
            memcpy(e->outbuf + e->outpos, j->sei, nsei);
            e->nals[cnt].naltype = KS265_NAL_SUFFIX_SEI; e->nals[cnt].tid = 0; e->nals[cnt].iSize = (int)nsei; e->nals[cnt].pts = j->pts; e->nals[cnt].pPayload = e->outbuf + e->outpos;
            e->outpos += nsei;
            ++cnt;
        }
        if (out) { out->iSliceType = j->kind == 'I' ? 2 : j->kind == 'P' && !j->gpb ? 1 : 0; out->poc = j->disp; out->pts = j->pts; out->dts = j->pts; }
        if (e->pool_on) {                                               /* the picture's reconstruction leaves the ring with it: the caller of this function hands it out, or stashes it */
            const ReconRef ref = {e->lane_idx, j->rslot, j->disp, j->kind == 'I' ? 2 : j->kind == 'P' && !j->gpb ? 1 : 0, j->pts};
            if (recon_list_push(&e->taken, &ref)) err = QY_OUTOFMEMORY;
        }
        e->st.frames++; e->st.bytes += (long long)need; e->st.host_write_ms += j->t_write_ms;
        e->st.lat_gpu_ms += j->t_event - j->t_submit; e->st.lat_queue_ms += j->t_taken - j->t_submit;
        if (j->kind == 'I') { e->st.key_wall_ms += j->t_done - j->t_event; e->st.key_cpu_ms += j->t_write_ms; e->st.keys++; }
        if (j->key_headers && e->cfg.bHeaderBeforeKeyframe) e->st.bytes += e->hdr_len;
        if (e->cfg.calcPsnr) {
            for (int k = 0; k < 3; ++k) e->st.sse[k] += (double)j->sse[k];
            if (e->cfg.calcPsnr >= 2) {
                const double np[3] = {(double)e->srcW * e->srcH, (double)e->srcW * e->srcH / 4, (double)e->srcW * e->srcH / 4};
                double ps[3];
                for (int k = 0; k < 3; ++k) ps[k] = j->sse[k] ? 10.0 * log10(255.0 * 255.0 * np[k] / (double)j->sse[k]) : 99.0;
                /* appencoder's -psnr 2 table: `poc slice bits psnrY psnrU psnrV qp`, tab separated, one header line */
                if (!e->psnr_hdr) { e->psnr_hdr = 1; logf_(2, e->log_level, "poc\tslice\tbits\tpsnr\t\t\tqp\n"); }
                logf_(2, e->log_level, "%d\t%c\t%ld\t%.4f\t%.4f\t%.4f\t%d\n", j->disp, j->gpb ? 'B' : j->kind /* (the slice type of the stream, as in the reference's lines) */, (long)j->nal_len * 8, ps[0], ps[1], ps[2], j->qp);
            }
        }
        if (e->ssim_on) {
            const double nw[3] = {(double)(e->W / 8) * (e->H / 8), (double)(e->W / 16) * (e->H / 16), (double)(e->W / 16) * (e->H / 16)};
            for (int k = 0; k < 3; ++k) {
                e->q_hi[k] += j->ssim[k] >> 30; e->q_lo[k] += j->ssim[k] & 0x3fffffff;
                e->q_last_ssim[k] = nw[k] > 0 ? (double)j->ssim[k] / 1073741824.0 / nw[k] : 0.0;
            }
            /* the reference prints nothing per picture with -ssim 2 (and its -psnr 2 table stays as it is: callers parse it): a line in this build's own style */
            if (e->cfg.calcSsim >= 2) logf_(2, e->log_level, "ks265enc: poc %d ssim %.4f %.4f %.4f\n", j->disp, e->q_last_ssim[0], e->q_last_ssim[1], e->q_last_ssim[2]);
        }
        e->q_last_poc = j->disp; e->q_seq = __atomic_add_fetch(&g_q_seq, 1, __ATOMIC_RELAXED);
        for (int k = 0; k < 3; ++k) e->q_last_sse[k] = e->cfg.calcPsnr ? (double)j->sse[k] : 0.0;
        if (e->md5 && e->md5_ring) {                                    /* `POC n MD5 y,u,v` in display order, like the reference's reconstruction output */
            memcpy(e->md5_ring[j->disp & 255], j->md5, sizeof j->md5); e->md5_have[j->disp & 255] = 1;
            while (e->md5_have[e->md5_next & 255]) {
                char (*m)[33] = e->md5_ring[e->md5_next & 255];
                logf_(2, e->log_level, "POC %d MD5 %s,%s,%s\n", e->md5_next, m[0], m[1], m[2]);
                e->md5_have[e->md5_next & 255] = 0; ++e->md5_next;
            }
        }
        rc_account(e);                                                  /* rate control: this picture's bits are on the books before its slot is reused */
        for (int i = 0; i < MAX_INPUT; ++i) if (e->in[i].used == IN_CODING && e->in[i].disp == j->disp) e->in[i].used = IN_FREE;
        j->used = 0;
        e->job_head = (e->job_head + 1) % e->ring; --e->njobs; ++taken;
        if (cnt >= (int)(sizeof e->nals / sizeof e->nals[0]) - 5) break;
    }
    if (taken) pthread_cond_broadcast(&e->cv_done);                    /* the scheduler thread may be waiting for ring space */
    pthread_mutex_unlock(&e->mu);
    *pNals = e->nals; *n = cnt;
    if (pics) *pics = taken;
    return err;
}

/* the reference's line behind `bitrate, psnr:` (or alone with -psnr 0), byte for byte its format (tests/golden/ssim_ref.npz): kbit/s, then the mean over the pictures of
 * every plane's mean over its windows.  hi / lo: the summed fixed-point window sums, hi x 2^30 + lo */
static double ssim_mean(long long hi, long long lo, double windows, long frames) { return windows > 0 && frames ? ((double)hi + (double)lo / 1073741824.0) / (windows * (double)frames) : 0.0; }
/* the end-of-run summary of a lane, or of all lanes of a handle: `bitrate, psnr:` (-psnr), then the ssim line (-ssim) */
static void run_summary(const Enc *e, long frames, long long bytes, const double sse[3], const long long hi[3], const long long lo[3])
{
    if (!frames) return;
    const double kbps = bytes * 8.0 * e->cfg.frameRate / frames / 1000.0;
    if (e->cfg.calcPsnr) {
        const double np[3] = {(double)e->srcW * e->srcH, (double)e->srcW * e->srcH / 4, (double)e->srcW * e->srcH / 4};
        double ps[3];
        for (int k = 0; k < 3; ++k) ps[k] = sse[k] > 0 ? 10.0 * log10(255.0 * 255.0 * np[k] * frames / sse[k]) : 99.0;
        logf_(2, e->log_level, "bitrate, psnr: %.4f\t%.4f\t%.4f\t%.4f\n", kbps, ps[0], ps[1], ps[2]);
    }
    if (e->ssim_on) {
        const double nw[3] = {(double)(e->W / 8) * (e->H / 8), (double)(e->W / 16) * (e->H / 16), (double)(e->W / 16) * (e->H / 16)};
        logf_(2, e->log_level, "\t ssim: %.4f\t%.4f\t%.4f\t%.4f\n", kbps, ssim_mean(hi[0], lo[0], nw[0], frames), ssim_mean(hi[1], lo[1], nw[1], frames), ssim_mean(hi[2], lo[2], nw[2], frames));
    }
}

/* ------------------------------------------------------------------ opening and closing a lane
 * lane_resolve decides: it fills the fields of Enc that are decisions (Enc::plan: the ones only the steps below read) from the configuration, the CLI-level defaults and the
 * environment, logs what was narrowed, and calls no entry of the device library.  lane_open is the list of steps that create what the plan says - their order is itself a
 * measured result (tests/test_lane_open_cpu.py pins it).  Every open_* has its close_* beneath it, which frees what that step may have created and tolerates a step that never
 * ran or stopped half way (the calloc of Enc zeroed everything); lane_close is the list of those. */
#define ENV_UNSET (-2147483647 - 1)
static int env_int(const char *name, int dflt) { const char *s = getenv(name); return s ? atoi(s) : dflt; }
static int env_set(const char *name) { return getenv(name) != NULL; }
static void ev_free(ks265_ctx *c, void **ev) { if (*ev) ks265_event_destroy(c, *ev); *ev = NULL; }
static int lane_base_qp(const QY265EncConfig *cfg, int rc) { const int q = rc == 3 ? cfg->crf : cfg->qp; return q < 0 ? 0 : q > 51 ? 51 : q; }

static void lane_resolve(Enc *e, const QY265EncConfig *cfg, int device, int multi)
{
    e->cfg = *cfg; e->log_level = cfg->logLevel;
    e->srcW = cfg->picWidth; e->srcH = cfg->picHeight; e->W = (e->srcW + 7) & ~7; e->H = (e->srcH + 7) & ~7; e->ragged = e->W != e->srcW || e->H != e->srcH;
    e->me_method = cfg->me < 0 ? 1 : cfg->me > 2 ? 2 : cfg->me;        /* EPZS / Cross (-me 3 / 4) are not built: UMH instead */
    e->hex_thr = (e->me_method == 2 && (cfg->preset == QY265PRESET_SLOW || cfg->preset == QY265PRESET_SLOWER)) ? 16 : 0;   /* tME+0x368, SURVEY-measured */
    e->subme = cfg->subme < 0 ? 1 : cfg->subme > 2 ? 2 : cfg->subme;      /* 0 off, 1 fast, 2 square full (qy265enc.h:137): the reference's refinement, ks265_frame_cfg.subme */
    e->refs = cfg->refnum < 1 ? 1 : cfg->refnum > 4 ? 4 : cfg->refnum;
    e->use_sao = cfg->sao > 0; e->use_df = g_cli.df; e->fixqp = g_cli.fixqp; e->md5 = g_cli.md5;
    e->gop_b = cfg->bframes < 0 ? (cfg->latency == QY265LATENCY_DEFAULT ? 7 : 0) : cfg->bframes;
    /* the pyramid: the SDK's default GOP (8), and - as in the reference, whose -psnr 2 lines show it - explicit -bframes 7 (the same) and -bframes 3: anchors 4 apart, the middle
     * picture a reference B at Q + 2, the two outer ones non-reference B at Q + 3 (appencoder -bframes 3 -qp 27: 28 / 29 / 30 / 30; until round 4 ours was P + 3 plain B at Q + 2).
     * -bframes 1 / 2: the reference codes both as anchors 2 apart with one B picture at Q + 2; ours: P + n plain B at Q + 2 */
    e->hier = e->gop_b == 7 || cfg->bframes == 3;
    /* with B pictures the anchors keep one reference; round 5: the B pictures of the pyramid search up to -ref pictures per list (ks265_encode_picture_b_mref: config 5 = -preset
     * veryslow resolves to 4 / 4) - of the pictures the mini-GOP keeps anyway (gop_plan), so the reference picture sets do not change */
    e->refs_b = e->hier ? e->refs : 1;
    if (e->gop_b > 0) e->refs = 1;
    /* round 6: -ref0 (-preset slow resolves to ref 1 / ref0 3): the anchors of a pyramid search the last ref0 anchors of their GOP (ks265_encode_picture_mref, list 0
     * nearest first = the default list construction); the older anchors stay in every reference picture set in between.  KS265_REF0 overrides (experiments: 1 = round 5's anchors) */
    const int ref0 = env_int("KS265_REF0", cfg->ref0);
    e->refs0 = e->hier ? (ref0 < 1 ? 1 : ref0 > 4 ? 4 : ref0) : 1;
    /* `gpb` (ks265_enc_set_default, KS265_GPB overrides): in force where an anchor can see two anchors - with B pictures and -ref0 > 1; IPPP and zero latency have no such anchors */
    e->gpb = env_int("KS265_GPB", g_cli.gpb) != 0 && e->gop_b > 0 && e->refs0 > 1;
    e->base_qp = lane_base_qp(cfg, cfg->rc);
    e->iper = cfg->iIntraPeriod;
    e->coded_upto = -1; e->gop_end = e->gop_end_seen = -1;
    /* the SDK's config has no device field: the lane's GPU comes from the handle (KS265_DEVICE: one GPU, default 0; KS265_GPUS / KS265_DEVICES: closed GOPs dealt
     * to lanes on several GPUs, QY265EncoderOpen) */
    e->dev_id = device; e->multi = multi;
    long ncpu = sysconf(_SC_NPROCESSORS_ONLN);
    e->nthreads = cfg->threads > 0 ? cfg->threads : (int)(ncpu > 0 ? ncpu : 4);
    if (e->nthreads > 64) e->nthreads = 64;
    const int ps = e->ct_preset = (int)cfg->preset < 0 || (int)cfg->preset > 8 ? QY265PRESET_SLOW : (int)cfg->preset;   /* the sub-pel knobs and cuTree's tables follow it */

    e->rdoq_on = cfg->rdoq == 2;                                      /* asked for by name (QY265ConfigParse); the presets' rdoq 1 = this build's seam */
    if (e->rdoq_on) logf_(2, e->log_level, "ks265enc: -rdoq 1: the luma transform blocks of inter CUs go through the reference's rdoQuant (bit tables from the context states of the stream, %d pictures behind)\n", RC_LAG + 1);
    if (cfg->transskip) logf_(1, e->log_level, "ks265enc: transskip is accepted but not implemented by the pixel path\n");
    if (cfg->tuInter > 1) logf_(1, e->log_level, "ks265enc: -intertu %d runs as -intertu 1 (the residual quadtree of inter CUs one level deep)\n", cfg->tuInter);
    if (cfg->tuIntra > 0) logf_(2, e->log_level, "ks265enc: -intratu is accepted but not implemented (intra CUs carry one transform unit)\n");
    if (cfg->iAqMode > 1) logf_(1, e->log_level, "ks265enc: -aq %d runs as -aq 1 (block variance, the mode of the reference's calcFrameAdaptQuant)\n", cfg->iAqMode);
    if (cfg->part && e->refs > 1) logf_(1, e->log_level, "ks265enc: -part 1 (2NxN / Nx2N partitions of 64 / 32 / 16 CUs) acts on P and B pictures with one reference picture per list; multi-reference P pictures keep 2Nx2N\n");
    /* options whose VALUE is narrowed (SURVEY.md 8(a) config 5 = -preset veryslow: subme 2, part 1, ref 4): said once, never silently */
    if (cfg->refnum > 4) logf_(1, e->log_level, "ks265enc: -ref %d runs as -ref 4\n", cfg->refnum);
    if (e->gop_b > 0 && cfg->refnum > 1 && !e->hier) logf_(1, e->log_level, "ks265enc: -ref %d with plain (non-pyramid) B pictures runs as one reference per list\n", cfg->refnum);
    if (e->hier && e->refs_b > 1) logf_(1, e->log_level, "ks265enc: B pictures search up to %d pictures per list (list 0: the nearest coded pictures before, list 1: after)\n", e->refs_b);
    if (e->hier && cfg->ref0 > 4) logf_(1, e->log_level, "ks265enc: -ref0 %d runs as -ref0 4\n", cfg->ref0);
    if (!e->hier && e->gop_b > 0 && cfg->ref0 > 1) logf_(1, e->log_level, "ks265enc: -ref0 %d with plain (non-pyramid) B pictures runs as one reference for the anchors\n", cfg->ref0);
    if (e->hier && e->refs0 > 1) logf_(2, e->log_level, "ks265enc: the anchors of the pyramid search the last %d anchors (-ref0)\n", e->refs0);
    if (cfg->rc == 5 || cfg->vbv_buffer_size) logf_(1, e->log_level, "ks265enc: CVQ / VBV are not implemented; running the plain controller\n");

    memset(&e->fcfg, 0, sizeof e->fcfg);
    e->fcfg.width = e->W; e->fcfg.height = e->H; e->fcfg.qp = e->base_qp; e->fcfg.lambda_q4 = kLambdaQ4[e->base_qp];
    e->fcfg.me_range = cfg->searchrange < 1 ? 64 : cfg->searchrange > 64 ? 64 : cfg->searchrange;
    e->fcfg.me_method = e->me_method; e->fcfg.subme = e->subme; e->fcfg.deblock = e->use_df;
    /* -sao (qy265enc.h:143: 1 / 2 faster, 3 usual, 4 complex): 3 given BY NAME = the reference's own decision on its -sao 4 path - band offset + the 0 / 90 degree edge classes priced by its pinned
     * estimation functions, rates and lambda table (ks265_frame_cfg.sao = 2: CEncSao::modeDecisionBoEo01 enc@0x4af300 without the merge candidates); every other level > 0 = this build's
     * rule over all four edge classes + band offset (the presets' -sao 4: 2.7 - 4.6 % fewer bytes at equal PSNR-Y than level 3, which buys 0.8 - 1.9 dB of chroma: DESIGN.md) */
    e->fcfg.sao = cfg->sao == 6 ? 3 : cfg->sao == 5 ? 2 : e->use_sao;   /* (5 = -sao 3 BY NAME or -sao-ref 1, 6 = -sao-ref 2: + the merge candidates, QY265ConfigParse; the presets' 3 is the build's rule) */
    /* the sub-pel refinement's knobs follow the preset, as in the reference */
    e->fcfg.sub_satd = kPresetSubme[ps].satd; e->fcfg.sub_thr = kPresetSubme[ps].thr; e->fcfg.sub_flat = kPresetSubme[ps].flat;
    e->fcfg.sub_cap = kPresetSubme[ps].cap; e->fcfg.sub_cap_step = kPresetSubme[ps].cap_step; e->fcfg.sub_diag_fast = kPresetSubme[ps].diag_fast;
    e->fcfg.bframes = e->gop_b; e->fcfg.refs = e->refs > e->refs_b ? e->refs : e->refs_b; if (e->refs0 > e->fcfg.refs) e->fcfg.refs = e->refs0; e->fcfg.me_hex_thr = e->hex_thr;
    e->fcfg.sdh = 1;                                                    /* the reference's streams have sign_data_hiding_enabled_flag = 1 at every preset */
    e->fcfg.pre_search = 1;                                             /* stage A0: pyramid pre-search vectors as start candidates of the integer search */
    e->fcfg.merge = 1;                                                  /* stage C2: merge pass on the motion field (pictures with one reference per list) */
    e->fcfg.propagate = env_int("KS265_PROPAGATE", 1) & 3;              /* stage A2: rounds of vector propagation between neighbouring PUs after every
                                                                         * integer search (measured with one round: - 21 .. - 23 % bytes of the P / B pictures; the variable is a measuring aid) */
    e->fcfg.intra_inter = 1;                                            /* P / B pictures may hold intra CUs (uncovered regions, occlusions); 2 = none of 8x8: measured + 1.6 % bits, no faster */
    e->fcfg.rdo = 4;                                                    /* coefficient-group pruning at lambda x 1 (ks265_frame_cfg.rdo): supersedes the coefficient decimation of round 2 */
    e->lean_b = env_int("KS265_LEAN_B", 1);                             /* non-reference B pictures without intra candidates / joint refinement / SAO (GopPic::lean) */
    e->fcfg.skip_rd = env_int("KS265_SKIP_RD", 1) & 3;                  /* stage D2 (round 6): after the reconstruction of a B picture, nodes whose merge candidate without
                                                                         * residual is the cheaper coding - on the coded distortion - become one CU (ks265_frame_cfg.skip_rd; 2 = P pictures
                                                                         * too, where it gains nothing measurable; the variable is a measuring aid) */
    e->fcfg.tu_inter = cfg->tuInter > 0 ? 1 : 0;                        /* -intertu N (tuInter; veryslow 1, placebo 2): the residual quadtree of inter CUs ONE level deep (ks265_frame_cfg.tu_inter); deeper values run as 1 */
    e->fcfg.part = cfg->part ? 1 : 0;                                   /* -part 1 (slower, veryslow, placebo): 2NxN / Nx2N prediction units in P and B pictures (ks265_frame_cfg.part) */
    e->fcfg.bi_refine = env_int("KS265_BI_REFINE", cfg->preset >= QY265PRESET_SLOWER && cfg->preset <= QY265PRESET_PLACEBO ? 2 : 0);   /* 2 (round 5): after the CU decision, for the CUs it chose; 1 = for every PU of the quadtree.  End of round 6: up to -preset slow it is off - measured on the MI355X at 1080p and 2160p it COSTS 0.5 - 0.7 % bytes at equal PSNR-Y (it lowers the Hadamard cost of residuals the quantiser drops, and pays vector bits) and 134 us per B picture; the presets that trade speed for tools (slower .. placebo) keep it */                                              /* B pictures: joint refinement of the bi-predictive pair (motionSearchBI enc@0x484910) */

    /* the pipeline's switches */
    e->plan.srcq = !env_set("KS265_NO_SPLIT");
    e->copy_mb = env_int("KS265_COPYOUT_MB", -1);
    e->key_overlap = !env_set("KS265_NO_KEY_OVERLAP");
    e->plan.key_prio = env_int("KS265_KEY_PRIO", 1);                    /* the key picture's wavefront must run underneath the P pictures, not behind them */
    e->plan.anc_prio = env_int("KS265_ANC_PRIO", 0);
    { const int sp = env_int("KS265_PIC_SPACER", 0); e->plan.spacer = sp > 0 ? (size_t)sp : 0; }
    e->ssim_on = cfg->calcSsim != 0 && ks265_ssim_picture && ks265_ssim_picture_on;
    if (cfg->calcSsim && !e->ssim_on) logf_(2, e->log_level, "ks265enc: SSIM is unavailable: the device library has no ks265_ssim_picture (-ssim is ignored, no ssim line)\n");
    /* `hash` (ks265_enc_set_default, KS265_HASH overrides; a value the setter would refuse counts as off) */
    const int hash_req = env_int("KS265_HASH", g_cli.hash);
    e->hash_on = (hash_req == 2 || hash_req == 3) && ks265_picture_hash && ks265_picture_hash_on ? hash_req : 0;
    if ((hash_req == 2 || hash_req == 3) && !e->hash_on)                 /* (once per handle: the lanes behind the first log errors only) */
        logf_(2, e->log_level, "ks265enc: picture hash is unavailable: the device library has no ks265_picture_hash (hash is ignored, no SEI messages)\n");
    e->aq_on = cfg->iAqMode != 0 && cfg->fAqStrength > 0;
    /* cuTree: -rc 3 (CRF) with the reference's -cutree 1 (its default), B pictures (with -bframes 0 the reference runs no tree: TEncParam+0x388 = 0, every offset it leaves is zero)
     * and a lookahead (not -lookahead 0, not zero latency): a QP per CTU from the lookahead window */
    e->ct_on = cfg->rc == 3 && g_cli.cutree && e->gop_b > 0 && cfg->lookahead != 0 && cfg->latency != QY265LATENCY_ZERO && e->W >= 64 && e->H >= 64 && !env_set("KS265_NO_CUTREE");
    {   /* how far behind a key picture / a mini-GOP's anchor the window reaches - measured inside the reference (the calcFrameCost calls of every batch, -bframes 3): veryfast 8,
         * fast / medium 12, slow / veryslow 60, -lookahead 20: 16 - i.e. a queue of L pictures (12 / 16 / 64 by preset, or -lookahead N) in whole mini-GOPs: ((L - 1) / span) span */
        const int L = cfg->lookahead > 0 ? cfg->lookahead : e->ct_preset <= 2 ? 12 : e->ct_preset <= 4 ? 16 : 64, span = e->gop_b + 1;
        e->ct_depth = ((L - 1) / span) * span;
    }
    if (e->ct_depth < e->gop_b + 1) e->ct_depth = e->gop_b + 1;
    if (e->ct_depth > CT_RING - 40) e->ct_depth = CT_RING - 40;
    /* `roi` (ks265_enc_set_default, KS265_ROI overrides): refused - logged, the switch then off - without the entries in the device library and with lanes on several GPUs
     * (multi == 2: the caller's maps lie on ONE device) */
    const int roi_req = env_int("KS265_ROI", g_cli.roi) != 0;
    const int roi_lib = ks265_roi_validate && ks265_roi_reduce && ks265_roi_ctu_map && ks265_wait_external && ks265_external_wait_event;
    e->roi_on = roi_req && roi_lib && multi != 2;
    if (roi_req && !e->roi_on)
        logf_(2, e->log_level, "ks265enc: ROI maps are unavailable: %s (roi is ignored)\n", !roi_lib ? "the device library has no ks265_roi_reduce" : "the handle's GOP lanes run on several GPUs");
    e->qmap_on = e->aq_on || e->ct_on || e->roi_on;
    e->plan.qmap_path = e->qmap_on ? getenv("KS265_DUMP_QPMAP") : NULL;
    if (e->ct_on) {                                                    /* the lookahead window's pictures: half size, in blocks of 8 or 16 samples */
        e->ct_w = e->W / 2; e->ct_h = e->H / 2;
        e->ct_lg = (kCtPreset[ps].lg4 || (long)e->W * e->H >= 1280L * 720) ? 4 : 3;
        const int bs = 1 << e->ct_lg;
        e->ct_nx = (e->ct_w + bs - 1) / bs; e->ct_ny = (e->ct_h + bs - 1) / bs;
        e->ct_pad = 40 + bs;                                               /* the search leaves the picture by at most merange / 2 + 1 = 33; the last block row / column may overhang it */
        e->ct_stride = (e->ct_w + 2 * e->ct_pad + 63) & ~63;
        logf_(1, e->log_level, "ks265enc: -rc 3: cuTree over a lookahead of %d pictures (%d x %d blocks of %d half-size samples; -cutree 0 / -lookahead 0 switch it off): QP per CTU = picture QP + the tree's mean offset\n",
              e->ct_depth, e->ct_nx, e->ct_ny, 1 << e->ct_lg);
    }
    if (e->aq_on && !e->ct_on) { e->aq_nx = (e->W + 15) / 16; e->aq_ny = (e->H + 15) / 16; }       /* blocks that hang over the picture read its padding (replicated edges) */
    e->ndpb = e->hier ? 10 : e->gop_b ? 4 : e->refs + 2;
    for (int i = 0; i < MAX_DPB; ++i) e->dpb_poc[i] = NO_PIC;
    const int graph_asked = env_set("KS265_GRAPH");
    e->use_graph = graph_asked;                                         /* opt-in since round 4: launch by launch is faster on this runtime (843 against 817 pictures/s, 2160p IPPP) and the split pipeline needs the launches apart */
    if (e->qmap_on) e->use_graph = 0;                                    /* (a captured picture would replay one map) */
    if (e->rdoq_on) {
        e->use_graph = 0;                                                /* (a captured picture would replay one set of tables) */
        /* rdoQuant's two lambdas by QP (luma weights 256 / 256 = -rdoql / -rdoqls of the reference): (int64)(weight x 0.85 x 2^((qp - 12) / 3) + 0.5) */
        for (int q = 0; q < 52; ++q) { const double lam = 0.85 * pow(2.0, (q - 12) / 3.0); e->rq_lam[q] = e->rq_lam[52 + q] = (int64_t)(256 * lam + 0.5); }
    }
    e->split = e->plan.srcq && !e->use_graph;                           /* (the graph experiment leaves the split pipeline's source pictures allocated and unused) */
    /* opt-in (KS265_ANCHOR_LANE=1): measured on the MI355X at 2160p, default GOP - 561 pictures/s without, 568 with the lane at normal stream priority, 440 at high priority
     * (and 382 before the anchor waited for its upload directly); with 8 hardware queues (GPU_MAX_HW_QUEUES) 449 without and 515 with.  The kernels of a picture fill the
     * device: an anchor running beside B pictures slows them by what it gains */
    e->anc_on = e->hier && e->refs0 == 1 && e->key_overlap && !e->qmap_on && !e->use_graph && env_int("KS265_ANCHOR_LANE", 0) > 0;

    /* `devrecon` (ks265_enc_set_default, KS265_DEVRECON overrides): every picture's reconstruction is packed into a pool slot and stays fetchable on the device until the call
     * after the one that handed it out.  Refused - logged, the switch then off - without the way back in the device library, with lanes on several GPUs (multi == 2: the
     * caller fetches on ONE device) and with the graph experiment (a captured picture would replay one slot) */
    const int rec_req = env_int("KS265_DEVRECON", g_cli.devrecon) != 0;
    const int rec_lib = ks265_output_convert && ks265_output_validate && ks265_set_stream;
    e->devrecon = rec_req && rec_lib && multi != 2 && !graph_asked;
    if (rec_req && !e->devrecon)
        logf_(2, e->log_level, "ks265enc: device reconstruction is unavailable: %s (devrecon is ignored)\n",
              !rec_lib ? "the device library has no ks265_output_convert" : multi == 2 ? "the handle's GOP lanes run on several GPUs" : "the KS265_GRAPH experiment replays captured pictures");
    /* `analysis` (ks265_enc_set_default, KS265_ANALYSIS overrides): every picture's analysis block is packed into its pool slot and stays fetchable as devrecon's picture does;
     * refused for the same three reasons */
    const int an_req = env_int("KS265_ANALYSIS", g_cli.analysis) != 0;
    const int an_lib = ks265_analysis_bytes && ks265_analysis_pack && ks265_analysis_validate && ks265_analysis_export && ks265_set_stream;
    e->analysis = an_req && an_lib && multi != 2 && !graph_asked;
    if (an_req && !e->analysis)
        logf_(2, e->log_level, "ks265enc: analysis is unavailable: %s (analysis is ignored)\n",
              !an_lib ? "the device library has no ks265_analysis_pack" : multi == 2 ? "the handle's GOP lanes run on several GPUs" : "the KS265_GRAPH experiment replays captured pictures");
    e->pool_on = e->devrecon || e->analysis;

    /* the temporal filter on the way in: vpp_denoise 1 / 2 / 3 = (thr, weight) (6, 16) / (10, 20) / (16, 24); vpp_recur_filter v > 0 replaces the weight by round(v) in 1 .. 30
     * and, alone, runs at thr 10 (lane_open has judged both fields) */
    e->dn_on = cfg->vpp_denoise > 0 || cfg->vpp_recur_filter > 0;
    if (e->dn_on) {
        static const int kDnThr[4] = {10, 6, 10, 16}, kDnWeight[4] = {20, 16, 20, 24};
        const int lv = cfg->vpp_denoise & 3, v = (int)(cfg->vpp_recur_filter + 0.5);
        e->dn_cfg.thr = kDnThr[lv];
        e->dn_cfg.weight = cfg->vpp_recur_filter > 0 ? (v < 1 ? 1 : v > 30 ? 30 : v) : kDnWeight[lv];
    }

    /* edge / colour enhancement on the way in: vpp_edge 1 / 2 / 3 = (gain in 1/16, core, limit, over) (8, 2, 8, 2) / (16, 2, 16, 4) / (24, 3, 24, 8); vpp_color 1 / 2 / 3 =
     * colour gain 8 / 16 / 32 (lane_open has judged both fields) */
    e->en_on = cfg->vpp_edge > 0 || cfg->vpp_color > 0;
    if (e->en_on) {
        static const ks265_enhance_cfg kEdge[4] = {{0, 0, 0, 0, 0}, {8, 2, 8, 2, 0}, {16, 2, 16, 4, 0}, {24, 3, 24, 8, 0}};
        static const int kColor[4] = {0, 8, 16, 32};
        e->en_cfg = kEdge[cfg->vpp_edge & 3];
        e->en_cfg.color_gain = kColor[cfg->vpp_color & 3];
    }

    /* local contrast on the way in (tests/hdr_ref.py params(), restated with its expression order; lane_open has judged the fields).  A field left at 0 takes this build's
     * default - strength 1.0, iter 3, sigma_s 20, sigma_r 15 (a percentage of the 8-bit range): untuned choices */
    e->hdr_on = cfg->vpp_hdr == 1;
    if (e->hdr_on) {
        const double strength = cfg->vpp_hdr_strength != 0 ? cfg->vpp_hdr_strength : 1.0, sigma_s = cfg->vpp_hdr_sigma_s != 0 ? cfg->vpp_hdr_sigma_s : 20.0,
                     sigma_r = cfg->vpp_hdr_sigma_r != 0 ? cfg->vpp_hdr_sigma_r : 15.0;
        const int n = cfg->vpp_hdr_iter ? cfg->vpp_hdr_iter : 3;
        const double sl = floor(1600 * sigma_s / (255 * sigma_r) + 0.5);
        memset(&e->hdr_cfg, 0, sizeof e->hdr_cfg);
        e->hdr_cfg.gain = (int)floor(16 * strength + 0.5);
        e->hdr_cfg.iters = n;
        e->hdr_cfg.slope = sl > 4096 ? 4096 : (int)sl;
        for (int i = 1; i <= n; ++i) {
            const int rad = (int)floor(16 * (3 * sigma_s * pow(2.0, n - i) / sqrt(pow(4.0, n) - 1)) + 0.5);
            e->hdr_cfg.radius[i - 1] = rad < 16 ? 16 : rad;
        }
    }

    /* the lookahead and the two optional streams */
    /* no -lookahead on the command line and the SDK's default GOP (hierarchical B, 8): the slice-type decision runs by itself (round 4: it costs a search of the half-size
     * picture every fourth picture, and the caller does not wait for it) - the reference's adaptive BiPredFrames is on by default as well.  -lookahead 0 switches it off. */
    e->la_auto = cfg->lookahead < 0 && e->hier && e->gop_b == 7 && !env_set("KS265_NO_AUTO_LOOKAHEAD");
    e->plan.la_wanted = cfg->lookahead > 0 || e->la_auto;
    e->plan.la_order = env_int("KS265_LA_ORDER", 0);                    /* (experiments: 1 = fourth, 2 = last) */
    e->plan.la_prio = env_int("KS265_LA_PRIO", ENV_UNSET);
    e->la_w = (e->W / 2) & ~7; e->la_h = (e->H / 2) & ~7;              /* the analysis sees the picture without its last columns / rows when half the size is no multiple of 8 */
    if (e->plan.la_wanted && (e->la_w < 16 || e->la_h < 16)) { if (!e->la_auto) logf_(1, e->log_level, "ks265enc: -lookahead %d: the analysis needs a picture of at least 32 x 32: off\n", cfg->lookahead); }
    else if (e->plan.la_wanted) {
        /* how many pictures may wait for their analysis before the caller waits for the oldest one: five with one lane (the caller is paced by the output anyway); a GOP lane
         * takes a whole GOP in ahead of its pixel path - its analyses queue up behind two lanes' kernels, and a caller that waited for them fed 770 pictures/s (round 5) */
        const int keep = env_int("KS265_LA_KEEP", 0);
        e->la_keep = keep > 0 && keep < LA_QMAX - 8 ? keep : multi ? 48 : 5;
        e->la_on = 1; e->la_last_key = NO_PIC; e->la_prev_icost = -1; e->mg_adapt = e->hier;
    }
    if (!e->la_on) e->la_auto = 0;
    const int big = (size_t)e->W * e->H * 3 / 2 >= ((size_t)1 << 20), in_copy = env_set("KS265_INPUT_COPY");
    /* (not with KS265_GRAPH: the host-synchronous copy out of the caller's memory runs on the runtime's null stream from the CALLING thread, and while another thread has a capture open
     * that fails - 4 of 6 runs of the 2160p default GOP ended in QY_FAIL, 6 of 6 pass with the copying path; found and fixed at the end of round 6) */
    e->direct_in = !in_copy && !graph_asked && big && !(cfg->latency == QY265LATENCY_ZERO && !multi);
    e->hold_in = env_int("KS265_INPUT_HOLD", 0) > 0;
    /* how the upload out of the caller's memory runs.  4 (default): host-synchronous, on no stream of the lane's (ks265_memcpy_h2d_sync): the call returns when the picture is on the device.
     * 0 / -1 / 1 / 2 (experiments): asynchronously on a stream of its own created first / in front of the lookahead's / after the copy streams / last, waited for at the end of the call.
     * Measured at 2160p (profiles/r06_input_upload.txt): ANY stream more costs the two-lane default GOP a third of its rate (754 -> 515 .. 600 pictures/s: hardware queues are shared in
     * creation order) although the caller's input time falls to 0.33 ms; without one the default GOP codes 777 (copying path 758) and IPPP 1 028 (1 025), input 0.88 / 0.26 ms */
    const int upl_order = env_int("KS265_UPL_ORDER", 4);
    e->plan.upl_at = upl_order == -1 ? (!in_copy && big ? -1 : UPL_NONE) : e->direct_in && upl_order >= 0 && upl_order <= 2 ? upl_order : UPL_NONE;
    if (e->direct_in && upl_order == 4) e->direct_in = 2;              /* host-synchronous uploads: no stream of their own */
    else if (e->direct_in && e->plan.upl_at == UPL_NONE) e->direct_in = 0;
    e->plan.input_slots = env_int("KS265_INPUT_SLOTS", ENV_UNSET);
    e->plan.pinned_mb = env_int("KS265_PINNED_MB", 4096);

    /* the stream's parameter sets */
    memset(&e->scfg, 0, sizeof e->scfg);
    e->scfg.width = e->W; e->scfg.height = e->H; e->scfg.sao = e->use_sao; e->scfg.deblock = e->use_df;
    e->scfg.crop_right = e->W - e->srcW; e->scfg.crop_bottom = e->H - e->srcH;   /* the conformance window of a ragged size (0, 0 otherwise: the SPS as it always was) */
    e->scfg.sdh = e->fcfg.sdh;
    e->zero_latency = cfg->latency == QY265LATENCY_ZERO && e->gop_b == 0 && !e->la_on && !multi;
    e->scfg.cu_qp_delta = e->qmap_on;
    e->scfg.list_mod = e->gpb;                                          /* the anchors' two lists of past pictures are not the default construction (gop_plan) */
    e->scfg.tu_inter = e->fcfg.tu_inter;
    e->scfg.wpp = 1;                                                    /* CTU rows as substreams: what lets several writer threads share one picture */
    e->scfg.max_dec_pic_buffering = e->hier ? 10 : e->gop_b ? 4 : e->refs + 1; e->scfg.log2_max_poc_lsb = 16;
    /* pictures that precede a picture in decoding order and follow it in output order: the whole GOP for the hierarchy (7, as before), ONE (the anchor) for
     * P + n non-reference B whatever n is (-bframes 1..15) */
    e->scfg.max_num_reorder = e->hier ? e->gop_b : e->gop_b ? 1 : 0;
    /* what the GOP planner reads of all this (nothing above changes after this point) */
    e->rules = (GopRules){.gop_b = e->gop_b, .hier = e->hier, .refs = e->refs, .refs_b = e->refs_b, .refs0 = e->refs0, .gpb = e->gpb, .fixqp = e->fixqp, .lean_b = e->lean_b, .mg_adapt = e->mg_adapt};
    e->gs.mg4_until = -1;
}

/* the sizes that need the frame object's compact layout (cmp_off[7]): the ring of pictures in flight, the writer threads it can feed, the input slots */
static void lane_rings(Enc *e)
{
    const size_t fsz = (size_t)e->W * e->H * 3 / 2, npx = (size_t)e->W * e->H;
    /* ring of pictures in flight: a key picture's slice takes one writer thread many picture periods, and output is in coding order - the ring must
     * hold everything that is coded meanwhile, or the GPU idles behind it.  About 6 GB of records (pinned compact block + expanded level planes + pinned input), at least 24 and at most MAX_JOBS pictures. */
    e->ring = (int)(((size_t)6 << 30) / (e->cmp_off[7] + npx * 3 + fsz));
    if (e->ring > MAX_JOBS) e->ring = MAX_JOBS;
    if (e->ring < 24) e->ring = 24;
    if (e->nthreads > e->ring - 14) e->nthreads = e->ring - 14;               /* more writers than pictures that can be in flight would idle */
    /* input slots: the ring + a mini-GOP.  A GOP lane takes a whole GOP more: the caller hands the GOPs out in stream order, so a lane that could not hold its next GOP
     * while it is still coding the current one would make the caller wait - and the OTHER lanes, whose next GOPs come after, run dry (measured: lanes idle a third of
     * the time with ring + 32 slots) */
    e->nin = e->ring + 32 + (e->la_on ? 8 : 0) + (e->ct_on ? e->ct_depth : 0) + (e->multi ? (e->cfg.iIntraPeriod < 256 ? e->cfg.iIntraPeriod : 256) : 0);
    if (e->plan.input_slots != ENV_UNSET) e->nin = e->plan.input_slots;
    if (e->nin < e->ring + 32) e->nin = e->ring + 32;
    if (e->nin > MAX_INPUT) e->nin = MAX_INPUT;
    /* `devrecon`: a slot per picture of the ring - a picture holds its slot while it is in the ring, and the slots the last call handed out come back at the start of the next
     * one, before anything waits: with fewer slots than the ring the scheduler would wait for the caller with job slots free.  A GOP lane adds a GOP: the pictures of a GOP that is
     * not yet at the head of the output order leave the ring for the handle's stash and keep their slots there (KS265_DEVRECON_SLOTS: a count above the ring's, experiments) */
    if (e->pool_on) {
        e->plan.recon_slots = e->ring + (e->multi ? (e->cfg.iIntraPeriod < 128 ? e->cfg.iIntraPeriod : 128) : 0);
        const int asked = env_int("KS265_DEVRECON_SLOTS", 0);
        if (asked > e->ring) e->plan.recon_slots = asked;
        if (e->plan.recon_slots > RECON_POOL_MAX) e->plan.recon_slots = RECON_POOL_MAX;
    }
    {   /* pinned host memory is a machine-wide resource: a lane's input slots stay under KS265_PINNED_MB (default 4096 MB; the ring + one mini-GOP is the floor).  At 2160p
         * a slot is 12.4 MB: ring + 32 = 132 slots = 1.6 GB; a GOP lane at -iper 128 asks for 260 = 3.2 GB; eight GPUs with two lanes each = 52 GB without the cap */
        const long long budget = e->plan.pinned_mb * 1048576LL;
        const int fit = (int)(budget / (long long)fsz);
        if (e->nin > fit && fit >= e->ring + 32) {
            logf_(1, e->log_level, "ks265enc: %d input slots of %.1f MB would pin %.1f GB per lane: %d slots (KS265_PINNED_MB=%lld)\n", e->nin, fsz / 1048576.0, e->nin * (double)fsz / 1073741824.0, fit, budget / 1048576LL);
            e->nin = fit;
        } else if (e->nin > fit) {
            logf_(1, e->log_level, "ks265enc: the ring + one mini-GOP (%d input slots, %.1f GB pinned) is above KS265_PINNED_MB=%lld and is the floor\n", e->ring + 32, (e->ring + 32) * (double)fsz / 1073741824.0, budget / 1048576LL);
            e->nin = e->ring + 32;
        }
    }
}

/* the lookahead's stream (position 0: first; 1: behind the copy streams; 2: with the lookahead's objects - there also whatever position 0 could not create) and the uploads'
 * (plan.upl_at): each is created where the plan's position matches.  An uploads' stream that cannot be created means the copying path; the first position of the lookahead's
 * stream may fail, the others may not */
static int open_la_stream(Enc *e, int pos)
{
    if (!e->plan.la_wanted || e->ctx_la) return KS265_OK;
    if (pos == 0) { if (e->plan.la_order == 0 && ks265_create(&e->ctx_la, e->dev_id)) e->ctx_la = NULL; return KS265_OK; }
    if (pos == 1) return e->plan.la_order == 1 ? ks265_create(&e->ctx_la, e->dev_id) : KS265_OK;
    return e->plan.la_prio != ENV_UNSET ? ks265_create_prio(&e->ctx_la, e->dev_id, e->plan.la_prio) : ks265_create(&e->ctx_la, e->dev_id);
}
static void open_upl_stream(Enc *e, int pos)
{
    if (e->plan.upl_at == pos && ks265_create(&e->ctx_upl, e->dev_id)) { e->ctx_upl = NULL; if (e->direct_in == 1) e->direct_in = 0; }
}

static int open_early_streams(Enc *e) { open_upl_stream(e, -1); (void)open_la_stream(e, 0); open_upl_stream(e, 0); return KS265_OK; }

static int open_main(Enc *e)
{
    int r = ks265_create(&e->path[PATH_MAIN].ctx, e->dev_id);         /* KS265_NO_DEVICE -> QY_FAIL: there is no CPU fallback */
    if (!r) r = ks265_frame_geometry(&e->fcfg, &e->geom);
    if (!r) r = ks265_frame_create(main_ctx(e), &e->fcfg, &e->path[PATH_MAIN].frame);
    if (!r) r = ks265_frame_compact_layout(main_frame(e), e->cmp_off);
    if (!r) lane_rings(e);
    return r;
}
static void close_main(Enc *e) { if (main_frame(e)) ks265_frame_destroy(main_frame(e)); }

static int open_copy_streams(Enc *e)
{
    int r = ks265_create(&e->ctx_in, e->dev_id);
    if (!r) r = ks265_create(&e->ctx_out, e->dev_id);
    if (!r) open_upl_stream(e, 1);
    if (!r) r = open_la_stream(e, 1);
    return r;
}

static int open_pipeline(Enc *e)
{
    const size_t fsz = (size_t)e->W * e->H * 3 / 2;
    int r = KS265_OK;
    for (int k = 0; k < NPIPE && !r; ++k) {
        r = ks265_dev_malloc(main_ctx(e), (void **)&e->dev_in[k], fsz);
        if (!r) r = ks265_dev_malloc(main_ctx(e), (void **)&e->stg[k], e->cmp_off[7]);
        if (!r) r = ks265_memset_async(main_ctx(e), e->stg[k], 0, e->cmp_off[7]);   /* the header's running counters start at zero */
        if (!r) r = ks265_event_create(main_ctx(e), &e->ev_h2d[k]);
        if (!r) r = ks265_event_create(main_ctx(e), &e->ev_loaded[k]);
        if (!r) r = ks265_event_create(main_ctx(e), &e->ev_staged[k]);
        if (!r) r = ks265_event_create(main_ctx(e), &e->ev_drained[k]);
        if (!r) r = ks265_event_create(main_ctx(e), &e->ev_coded[k]);
        if (!r) r = ks265_event_create(main_ctx(e), &e->ev_packed[k]);
        if (!r && e->plan.srcq) r = pic_alloc(e, &e->srcq[k]);
    }
    return r;
}
static void close_pipeline(Enc *e)
{
    for (int k = 0; k < NPIPE; ++k) {
        ks265_dev_free(main_ctx(e), e->dev_in[k]); ks265_dev_free(main_ctx(e), e->stg[k]);
        ev_free(main_ctx(e), &e->ev_h2d[k]); ev_free(main_ctx(e), &e->ev_loaded[k]); ev_free(main_ctx(e), &e->ev_staged[k]);
        ev_free(main_ctx(e), &e->ev_drained[k]); ev_free(main_ctx(e), &e->ev_coded[k]); ev_free(main_ctx(e), &e->ev_packed[k]);
        pic_free(e, &e->srcq[k]);
    }
}

static int open_quality(Enc *e)
{
    int r = ks265_dev_malloc(main_ctx(e), (void **)&e->path[PATH_MAIN].dev_sse, 64);
    if (!r && e->ssim_on) r = ks265_dev_malloc(main_ctx(e), (void **)&e->path[PATH_MAIN].dev_ssim, 96);
    if (!r && e->hash_on) r = ks265_dev_malloc(main_ctx(e), (void **)&e->path[PATH_MAIN].dev_hash, 96);
    return r;
}
static void close_quality(Enc *e) { ks265_dev_free(main_ctx(e), e->path[PATH_MAIN].dev_sse); ks265_dev_free(main_ctx(e), e->path[PATH_MAIN].dev_ssim); ks265_dev_free(main_ctx(e), e->path[PATH_MAIN].dev_hash); }

/* what a QP per CTU needs: cuTree's stream and ring (ct_open), the maps of the pipeline's slots and of the key pictures, -aq's buffers where cuTree does not compute the offsets */
static int open_qmaps(Enc *e)
{
    int r = KS265_OK;
    if (e->plan.qmap_path) e->qmap_fd = open(e->plan.qmap_path, O_WRONLY | O_CREAT | O_APPEND, 0644);
    if (e->ct_on) r = ct_open(e);
    if (e->qmap_on) {
        for (int k = 0; k < NPIPE && !r; ++k) r = ks265_dev_malloc(main_ctx(e), (void **)&e->dev_qmap[k], (size_t)e->geom.ctu_cols * e->geom.ctu_rows);
        for (int q = 0; q < 2 && !r; ++q) r = ks265_dev_malloc(main_ctx(e), (void **)&e->dev_qmap_key[q], (size_t)e->geom.ctu_cols * e->geom.ctu_rows);
    }
    if (e->aq_on && !e->ct_on) {
        const size_t nb = (size_t)e->aq_nx * e->aq_ny;
        for (int q = PATH_MAIN; q <= PATH_KEY && !r; ++q) {
            r = ks265_dev_malloc(main_ctx(e), (void **)&e->path[q].aq_off, nb * 8);
            if (!r) r = ks265_dev_malloc(main_ctx(e), (void **)&e->path[q].aq_inv, nb * 2);
            if (!r) r = ks265_dev_malloc(main_ctx(e), (void **)&e->path[q].aq_scratch, 16);
        }
        e->path[PATH_ANC].aq_off = e->path[PATH_MAIN].aq_off; e->path[PATH_ANC].aq_inv = e->path[PATH_MAIN].aq_inv; e->path[PATH_ANC].aq_scratch = e->path[PATH_MAIN].aq_scratch;
    }
    return r;
}
static void close_qmaps(Enc *e)
{
    for (int q = PATH_MAIN; q <= PATH_KEY; ++q) { ks265_dev_free(main_ctx(e), e->path[q].aq_off); ks265_dev_free(main_ctx(e), e->path[q].aq_inv); ks265_dev_free(main_ctx(e), e->path[q].aq_scratch); }
    for (int k = 0; k < NPIPE; ++k) ks265_dev_free(main_ctx(e), e->dev_qmap[k]);
    for (int q = 0; q < 2; ++q) ks265_dev_free(main_ctx(e), e->dev_qmap_key[q]);
    if (e->qmap_fd >= 0) close(e->qmap_fd);
    ct_close(e);
}

static int open_dpb(Enc *e)
{
    int r = pic_alloc(e, &e->path[PATH_MAIN].src);
    for (int i = 0; i < e->ndpb && !r; ++i) r = pic_alloc(e, &e->dpb[i]);
    return r;
}
static void close_dpb(Enc *e)                                          /* (and the spacers in front of the lane's pictures: pic_alloc) */
{
    for (int i = 0; i < e->ndpb; ++i) pic_free(e, &e->dpb[i]);
    for (int i = 0; i < e->nspacer; ++i) ks265_dev_free(main_ctx(e), e->spacer[i]);
    pic_free(e, &e->path[PATH_MAIN].src);
}

/* a pixel path beside the main one (the key pictures', the anchors'): a stream of the given priority, a frame object on it, a source picture, the block of its SSE sums */
static int path_open(Enc *e, int which, int prio)
{
    PixPath *p = &e->path[which];
    int r = ks265_create_prio(&p->ctx, e->dev_id, prio);
    if (!r) r = ks265_frame_create(p->ctx, &e->fcfg, &p->frame);
    if (!r) r = pic_alloc(e, &p->src);
    if (!r) r = ks265_dev_malloc(main_ctx(e), (void **)&p->dev_sse, 64);
    if (e->path[PATH_MAIN].dev_ssim) p->dev_ssim = e->path[PATH_MAIN].dev_ssim + 4 * which;
    if (e->path[PATH_MAIN].dev_hash) p->dev_hash = e->path[PATH_MAIN].dev_hash + 8 * which;
    return r;
}
static void path_close(Enc *e, int which)                              /* the path's stream runs dry before its frame object goes (the contexts: last, lane_close) */
{
    PixPath *p = &e->path[which];
    if (p->ctx) ks265_synchronize(p->ctx);
    if (p->frame) ks265_frame_destroy(p->frame);
    pic_free(e, &p->src); ks265_dev_free(main_ctx(e), p->dev_sse);
}

static int open_key_path(Enc *e)
{
    if (!e->key_overlap) return KS265_OK;
    int r = path_open(e, PATH_KEY, e->plan.key_prio);
    if (!r) r = ks265_event_create(main_ctx(e), &e->ev_key);
    for (int i = 0; i < 2 && !r; ++i) { r = pic_alloc(e, &e->dpb[e->ndpb + i]); if (!r) r = ks265_event_create(main_ctx(e), &e->ev_firstp[i]); }
    return r;
}
static void close_key_path(Enc *e)
{
    for (int i = 0; i < 2; ++i) { pic_free(e, &e->dpb[e->ndpb + i]); ev_free(main_ctx(e), &e->ev_firstp[i]); }
    ev_free(main_ctx(e), &e->ev_key);
    path_close(e, PATH_KEY);
}

static int open_anchor_path(Enc *e)
{
    if (!e->anc_on) return KS265_OK;
    int r = path_open(e, PATH_ANC, e->plan.anc_prio);
    if (!r) r = ks265_event_create(main_ctx(e), &e->ev_anc);
    for (int i = 0; i < 8 && !r; ++i) r = ks265_event_create(main_ctx(e), &e->ev_mg[i]);
    for (int i = 0; i < 4 && !r; ++i) r = pic_alloc(e, &e->dpb[e->ndpb + 2 + i]);
    return r;
}
static void close_anchor_path(Enc *e)
{
    path_close(e, PATH_ANC);
    ev_free(main_ctx(e), &e->ev_anc);
    for (int i = 0; i < 8; ++i) ev_free(main_ctx(e), &e->ev_mg[i]);
    for (int i = 0; i < 4; ++i) pic_free(e, &e->dpb[e->ndpb + 2 + i]);
}

static int open_lookahead(Enc *e)
{
    if (!e->la_on) return KS265_OK;
    ks265_frame_cfg lc; memset(&lc, 0, sizeof lc);
    lc.width = e->la_w; lc.height = e->la_h; lc.qp = e->base_qp > 0 ? e->base_qp : 27; lc.lambda_q4 = kLambdaQ4[lc.qp < 52 ? lc.qp : 51]; lc.me_range = 32; lc.me_method = 1; lc.subme = 0;
    lc.bframes = 0; lc.refs = 1;
    int r = open_la_stream(e, 2);
    if (!r) r = ks265_frame_geometry(&lc, &e->geom_la);
    if (!r) r = ks265_frame_create(e->ctx_la, &lc, &e->frame_la);
    for (int i = 0; i < LA_RING && !r; ++i) {
        r = ks265_dev_malloc(e->ctx_la, (void **)&e->la_pic[i].y, (size_t)e->geom_la.bytes_y);
        if (!r) r = ks265_dev_malloc(e->ctx_la, (void **)&e->la_pic[i].u, (size_t)e->geom_la.bytes_c);
        if (!r) r = ks265_dev_malloc(e->ctx_la, (void **)&e->la_pic[i].v, (size_t)e->geom_la.bytes_c);
        if (!r) r = ks265_memset_async(e->ctx_la, e->la_pic[i].u, 128, (size_t)e->geom_la.bytes_c);     /* the analysis is luma only */
        if (!r) r = ks265_memset_async(e->ctx_la, e->la_pic[i].v, 128, (size_t)e->geom_la.bytes_c);
    }
    if (!r) r = ks265_dev_malloc(e->ctx_la, (void **)&e->la_cost_ws, (size_t)e->geom_la.ctu_cols * e->geom_la.ctu_rows * 85 * sizeof(uint32_t));
    if (!r) r = ks265_dev_malloc(e->ctx_la, (void **)&e->la_dev_out, LA_FLY * 128);
    if (!r) r = ks265_host_malloc(e->ctx_la, (void **)&e->la_host_out, LA_FLY * 128);
    for (int i = 0; i < LA_FLY && !r; ++i) r = ks265_event_create(e->ctx_la, &e->la_evs[i]);
    return r;
}
static void close_lookahead(Enc *e)                                    /* (the stream may be all there is: it is created first, before the main context) */
{
    if (!e->ctx_la) return;
    ks265_synchronize(e->ctx_la);
    for (int i = 0; i < LA_RING; ++i) { ks265_dev_free(e->ctx_la, e->la_pic[i].y); ks265_dev_free(e->ctx_la, e->la_pic[i].u); ks265_dev_free(e->ctx_la, e->la_pic[i].v); }
    ks265_dev_free(e->ctx_la, e->la_cost_ws); ks265_dev_free(e->ctx_la, e->la_dev_out); ks265_host_free(e->ctx_la, e->la_host_out);
    for (int i = 0; i < LA_FLY; ++i) ev_free(e->ctx_la, &e->la_evs[i]);
    if (e->frame_la) ks265_frame_destroy(e->frame_la);
    ks265_destroy(e->ctx_la);
    e->ctx_la = NULL;
}

static int open_jobs(Enc *e)
{
    const size_t npx = (size_t)e->W * e->H;
    int r = KS265_OK;
    if (e->rdoq_on && !(e->rq_hist = (int32_t *)calloc((size_t)RQ_HIST * 1440, sizeof(int32_t)))) r = KS265_OUTOFMEMORY;
    for (int i = 0; i < e->ring && !r; ++i) {
        Job *j = &e->jobs[i];
        r = ks265_host_malloc(main_ctx(e), (void **)&j->cmp, e->cmp_off[7]);
        if (!r) {
            j->lvlbuf = (uint8_t *)calloc(npx * 3 + 64, 1);                 /* zero pages until a picture touches them */
            j->dirty = (uint64_t *)calloc((e->cmp_off[6] - e->cmp_off[5]) / 8 + 1, 8);
            if (!j->lvlbuf || !j->dirty) r = KS265_OUTOFMEMORY;
            j->cu8 = (ks265_cu8 *)(j->cmp + e->cmp_off[0]); j->sao = (ks265_sao_param *)(j->cmp + e->cmp_off[1]); j->sse = (uint64_t *)(j->cmp + e->cmp_off[2]);
            j->lvl[0] = (int16_t *)j->lvlbuf; j->lvl[1] = (int16_t *)(j->lvlbuf + npx * 2); j->lvl[2] = (int16_t *)(j->lvlbuf + npx * 2 + npx / 2);
        }
        if (!r && e->qmap_on) r = ks265_host_malloc(main_ctx(e), (void **)&j->qp_map, (size_t)e->geom.ctu_cols * e->geom.ctu_rows);
        if (!r && e->ssim_on) r = ks265_host_malloc(main_ctx(e), (void **)&j->ssim, 32);
        if (!r && e->hash_on) r = ks265_host_malloc(main_ctx(e), (void **)&j->hash, 32);
        if (!r && e->rdoq_on) r = ks265_host_malloc(main_ctx(e), (void **)&j->rq_host, 1440 * sizeof(int32_t) + 104 * sizeof(int64_t));
        if (!r) r = ks265_event_create(main_ctx(e), &j->ev);
        j->nal_cap = npx * 2 + 65536;
        j->nal = (uint8_t *)malloc(j->nal_cap);
        if (!j->nal) r = KS265_OUTOFMEMORY;
    }
    return r;
}
static void close_jobs(Enc *e)
{
    for (int i = 0; i < MAX_JOBS; ++i) {
        Job *j = &e->jobs[i];
        ks265_host_free(main_ctx(e), j->cmp); ks265_host_free(main_ctx(e), j->recon); ks265_host_free(main_ctx(e), j->qp_map); ks265_host_free(main_ctx(e), j->ssim); ks265_host_free(main_ctx(e), j->hash); ks265_host_free(main_ctx(e), j->rq_host); free(j->lvlbuf); free(j->dirty);
        ev_free(main_ctx(e), &j->ev);
        free(j->nal);
    }
    free(e->rq_hist);
}

static int open_inputs(Enc *e)
{
    const size_t fsz = (size_t)e->W * e->H * 3 / 2;
    int r = KS265_OK;
    for (int i = 0; i < e->nin && !r; ++i) r = ks265_host_malloc(main_ctx(e), (void **)&e->in[i].i420, fsz);
    /* with the lookahead every input slot has a twin on the device, uploaded on the lookahead's stream the moment the picture is handed in (nothing on that stream ever waits for
     * the pipeline: an upload enqueued on the copy-in stream, or anywhere on the copy engine behind that stream's uploads, sits behind the pipeline's back-pressure and the
     * analysis would see the picture 10 ms and more late); without it the picture is uploaded when it is scheduled, on the copy-in stream, as before.  One stream for both,
     * not a sixth: a stream more is a hardware queue shared with somebody (lane_open) */
    open_upl_stream(e, 2);
    if ((e->la_on && e->ctx_la) || e->direct_in || e->ragged || e->dn_on || e->en_on || e->hdr_on) {   /* (ragged, the denoiser, local contrast, the enhancement: the padded / filtered picture exists on the device only - every consumer reads the twin) */
        e->ctx_up = e->direct_in == 1 && e->ctx_upl ? e->ctx_upl : e->ctx_la ? e->ctx_la : main_ctx(e);
        reg_handle(main_ctx(e), 1);
        for (int i = 0; i < e->nin && !r; ++i) { r = ks265_dev_malloc(main_ctx(e), (void **)&e->in[i].dev, fsz); if (!r) r = ks265_event_create(e->ctx_up, &e->in[i].ev_up); }
        logf_(2, e->log_level, "ks265enc: %d input slots with a device twin each: %.2f GB of device memory per lane (KS265_INPUT_SLOTS / KS265_PINNED_MB bound the slot count)\n", e->nin, e->nin * (double)fsz / 1073741824.0);
    }
    if (e->ragged)                                                      /* every slot: the staging area of the picture as it came */
        for (int i = 0; i < e->nin && !r; ++i) r = ks265_dev_malloc(main_ctx(e), (void **)&e->in[i].raw, (size_t)e->srcW * e->srcH * 3 / 2);
    if (e->dn_on)                                                       /* the two history pictures */
        for (int k = 0; k < 2 && !r; ++k) r = ks265_dev_malloc(main_ctx(e), (void **)&e->dn_hist[k], fsz);
    if (e->en_on && e->en_cfg.edge_gain && (!e->dn_on || e->hdr_on) && !r)   /* the luma copy that the stencil reads (with the denoiser and without vpp_hdr: its history picture) */
        r = ks265_dev_malloc(main_ctx(e), (void **)&e->en_luma, (size_t)e->W * e->H);
    if (e->hdr_on && !r) {                                              /* the local-contrast filter's work buffer: what the device library asks for */
        e->hdr_bytes = ks265_input_hdr_work_bytes(e->W, e->H);
        r = e->hdr_bytes ? ks265_dev_malloc(main_ctx(e), &e->hdr_work, e->hdr_bytes) : KS265_NOTSUPPORTED;
    }
    if (e->roi_on) {                                                    /* every slot: the picture's record on the device, its pinned twin, the event behind its filling - on the upload stream there is, no stream more */
        const size_t nb = (size_t)e->geom.ctu_cols * e->geom.ctu_rows * sizeof(int32_t);
        if (!e->ctx_up) { e->ctx_up = e->ctx_la ? e->ctx_la : main_ctx(e); reg_handle(main_ctx(e), 1); }
        for (int i = 0; i < e->nin && !r; ++i) {
            r = ks265_dev_malloc(main_ctx(e), (void **)&e->in[i].roi_rec, nb);
            if (!r) r = ks265_host_malloc(main_ctx(e), (void **)&e->in[i].roi_host, nb);
            if (!r) r = ks265_event_create(e->ctx_up, &e->in[i].ev_roi);
        }
    }
    return r;
}
static void close_inputs(Enc *e)                                       /* (also what lane_enable_device_input added: twins, their events, the handle's count) */
{
    for (int k = 0; k < 2; ++k) if (e->dn_hist[k]) ks265_dev_free(main_ctx(e), e->dn_hist[k]);
    if (e->en_luma) ks265_dev_free(main_ctx(e), e->en_luma);
    if (e->hdr_work) ks265_dev_free(main_ctx(e), e->hdr_work);
    for (int i = 0; i < MAX_INPUT; ++i) { ks265_host_free(main_ctx(e), e->in[i].i420); ks265_dev_free(main_ctx(e), e->in[i].dev); ev_free(e->ctx_up, &e->in[i].ev_up);
                                          if (e->in[i].raw) ks265_dev_free(main_ctx(e), e->in[i].raw);
                                          ks265_dev_free(main_ctx(e), e->in[i].roi_rec); ks265_host_free(main_ctx(e), e->in[i].roi_host); ev_free(e->ctx_up, &e->in[i].ev_roi); }
}
static void close_input_streams(Enc *e)                                /* behind the lookahead (ctx_up may be its stream) */
{
    if (e->ctx_up) reg_handle(main_ctx(e), 0);
    if (e->ctx_upl) { ks265_synchronize(e->ctx_upl); ks265_destroy(e->ctx_upl); }
}

static int open_output(Enc *e)                                         /* host memory only: the parameter sets, the NAL buffer, the writers' job memory */
{
    e->hdr = (uint8_t *)malloc(512);
    if (e->hdr) {
        long a = ks265_write_vps(&e->scfg, e->hdr, 512), b = a > 0 ? ks265_write_sps(&e->scfg, e->hdr + a, 512 - (size_t)a) : -1, c = b > 0 ? ks265_write_pps(&e->scfg, e->hdr + a + b, 512 - (size_t)(a + b)) : -1;
        e->hdr_len = c > 0 ? a + b + c : -1;
        e->hdr_part[0] = a; e->hdr_part[1] = b; e->hdr_part[2] = c;
    }
    e->outcap = (size_t)e->W * e->H + 65536;
    e->outbuf = (uint8_t *)malloc(e->outcap);
    if (!e->hdr || e->hdr_len < 0 || !e->outbuf) return KS265_FAIL;
    for (int i = 0; i < e->ring; ++i) if (!(e->jobs[i].wpp = malloc(ks265_wpp_bytes(&e->scfg)))) return KS265_OUTOFMEMORY;   /* virtual until used */
    return KS265_OK;
}
static void close_output(Enc *e)
{
    for (int i = 0; i < MAX_JOBS; ++i) free(e->jobs[i].wpp);
    free(e->hdr); free(e->outbuf);
}

static int open_md5(Enc *e)                                            /* -md5 1: plane MD5s of every reconstructed picture */
{
    if (!e->md5) return KS265_OK;
    e->md5_ring = calloc(256, sizeof *e->md5_ring); e->md5_have = calloc(256, 1);
    return !e->md5_ring || !e->md5_have || lane_recon_on(e) ? KS265_OUTOFMEMORY : KS265_OK;
}
static void close_md5(Enc *e) { free(e->md5_ring); free(e->md5_have); }   /* (what lane_recon_on made goes with the jobs and in lane_close) */

/* `devrecon`: the pool's pictures and events.  No stream: a conversion runs IN the caller's stream, through a context that adopts it (ks265_enc_get_device_recon makes that
 * context at the first fetch) - measured at 2160p with two lanes, one more stream per lane, idle, cost 7.6 % (846 -> 781 pictures/s: it moves the streams of the lane opened
 * behind it to other hardware queues, as every stream more does - lane_open) */
static int open_devrecon(Enc *e)
{
    if (!e->pool_on) return KS265_OK;
    const size_t fsz = (size_t)e->W * e->H * 3 / 2, asz = e->analysis ? ks265_analysis_bytes(main_frame(e)) : 0;
    if (recon_pool_init(&e->rpool, e->plan.recon_slots)) return KS265_FAIL;
    int r = KS265_OK;
    for (int i = 0; i < e->rpool.n && !r; ++i) {
        if (e->devrecon) r = ks265_dev_malloc(main_ctx(e), (void **)&e->rslot[i].dev, fsz);
        if (!r) r = ks265_event_create(main_ctx(e), &e->rslot[i].ev_packed);
        if (!r && e->devrecon) r = ks265_event_create(main_ctx(e), &e->rslot[i].ev_read);
        if (!r && e->analysis) r = ks265_dev_malloc(main_ctx(e), (void **)&e->rslot[i].an, asz);
        if (!r && e->analysis) r = ks265_event_create(main_ctx(e), &e->rslot[i].ev_read_an);
    }
    if (!r && e->devrecon && e->ragged) {                               /* the window of a ragged lane's pictures: one scratch picture of the caller's size and the event that guards it */
        r = ks265_dev_malloc(main_ctx(e), (void **)&e->crop_scr, (size_t)e->srcW * e->srcH * 3 / 2);
        if (!r) r = ks265_event_create(main_ctx(e), &e->ev_crop);
    }
    if (e->devrecon)
        logf_(1, e->log_level, "ks265enc: device reconstruction: a pool of %d packed I420 pictures, %.1f MB of device memory per lane (the ring of %d pictures in flight%s)\n", e->rpool.n,
              e->rpool.n * (double)fsz / 1048576.0, e->ring, e->multi ? " + a GOP in the stash" : "");
    if (e->analysis)
        logf_(1, e->log_level, "ks265enc: analysis: a pool of %d blocks of %zu bytes, %.1f MB of device memory per lane (%s)\n", e->rpool.n, asz, e->rpool.n * (double)asz / 1048576.0,
              e->devrecon ? "the slots of the device reconstruction's pool" : e->multi ? "the ring of pictures in flight + a GOP in the stash" : "the ring of pictures in flight");
    return r;
}
static void close_devrecon(Enc *e)                                     /* a conversion still in flight on a stream of the caller's reads its slot: waited for, by its event (the context: last, lane_close) */
{
    for (int i = 0; i < RECON_POOL_MAX; ++i) if (e->rslot[i].read_on) (void)ks265_event_wait(main_ctx(e), e->rslot[i].ev_read);
    for (int i = 0; i < RECON_POOL_MAX; ++i) if (e->rslot[i].read_on_an) (void)ks265_event_wait(main_ctx(e), e->rslot[i].ev_read_an);
    for (int i = 0; i < RECON_POOL_MAX; ++i) { ks265_dev_free(main_ctx(e), e->rslot[i].dev); ev_free(main_ctx(e), &e->rslot[i].ev_packed); ev_free(main_ctx(e), &e->rslot[i].ev_read); }
    for (int i = 0; i < RECON_POOL_MAX; ++i) { ks265_dev_free(main_ctx(e), e->rslot[i].an); ev_free(main_ctx(e), &e->rslot[i].ev_read_an); }
    if (e->crop_used) (void)ks265_event_wait(main_ctx(e), e->ev_crop);
    if (e->crop_scr) { ks265_dev_free(main_ctx(e), e->crop_scr); e->crop_scr = NULL; }
    if (e->ev_crop) ev_free(main_ctx(e), &e->ev_crop);
    recon_list_free(&e->taken);
}

/* ks265_enc_enable_device_scale: the RGB sources' scratch picture, nothing else (the plans come with the sizes, on the caller's thread: lane_scale_plan) */
static int open_scale(Enc *e) { return ks265_dev_malloc(main_ctx(e), (void **)&e->sc_scratch, (size_t)e->sc_max_w * e->sc_max_h * 3 / 2); }
static void close_scale(Enc *e)
{
    for (int i = 0; i < SCALE_PLANS; ++i) if (e->sc_plan[i].plan) { (void)ks265_scale_plan_destroy(main_ctx(e), e->sc_plan[i].plan); e->sc_plan[i].plan = NULL; }
    ks265_dev_free(main_ctx(e), e->sc_scratch); e->sc_scratch = NULL;
}

static int open_threads(Enc *e)
{
    for (int i = 0; i < e->nthreads; ++i) { e->warg[i].e = e; e->warg[i].idx = i; if (pthread_create(&e->th[i], NULL, worker, &e->warg[i])) break; ++e->nth; }
    if (e->nth && !pthread_create(&e->disp, NULL, dispatcher, e)) e->disp_on = 1;
    if (e->disp_on && !pthread_create(&e->sched, NULL, scheduler, e)) e->sched_on = 1;
    return !e->nth || !e->disp_on || !e->sched_on ? KS265_FAIL : KS265_OK;
}
static void close_threads(Enc *e)
{
    if (!e->nth && !e->disp_on && !e->sched_on) return;
    pthread_mutex_lock(&e->mu); e->quit = 1; pthread_cond_broadcast(&e->cv_work); pthread_cond_broadcast(&e->cv_disp); pthread_cond_broadcast(&e->cv_sched); pthread_cond_broadcast(&e->cv_done); pthread_mutex_unlock(&e->mu);
    if (e->sched_on) pthread_join(e->sched, NULL);
    for (int i = 0; i < e->nth; ++i) pthread_join(e->th[i], NULL);
    if (e->disp_on) pthread_join(e->disp, NULL);
}

static void lane_close(Enc *e, int report)
{
    if (!e) return;
    close_threads(e);
    if (main_ctx(e)) {                                                 /* (without it nothing but the two early streams exists) */
        if (e->ctx_in) ks265_synchronize(e->ctx_in);
        ks265_synchronize(main_ctx(e));
        if (e->ctx_out) ks265_synchronize(e->ctx_out);
        if (report && e->la_on) logf_(1, e->log_level, "ks265enc: lookahead: %ld scene cuts, %ld blocks of 8 pictures coded as 4 + 4\n", e->la_cuts, e->la_mini4);
        if (report && e->la_on && e->in_disp) logf_(1, e->log_level, "ks265enc: lookahead, caller's ms per picture: launches + queue %.3f, of it waiting for results %.3f (%ld waits); pictures handed on by the scheduler thread: %ld\n",
                                                    e->la_t_take / e->in_disp, e->la_t_wait / e->in_disp, e->la_n_wait, e->la_n_poll);
        if (report && e->in_disp) logf_(1, e->log_level, "ks265enc: caller's back-pressure wait %.3f ms per picture\n", e->la_t_bp / e->in_disp);
        if (report) run_summary(e, e->st.frames, e->st.bytes, e->st.sse, e->q_hi, e->q_lo);
        close_devrecon(e);
        if (e->sc_on) close_scale(e);
        if (e->tm_plan) { (void)ks265_tonemap_plan_destroy(main_ctx(e), e->tm_plan); e->tm_plan = NULL; }
        close_jobs(e); close_inputs(e); close_dpb(e); close_key_path(e); close_anchor_path(e); close_pipeline(e);
        for (int i = 0; i < e->ngraph; ++i) ks265_graph_destroy(main_ctx(e), e->graph[i].exec);
        close_quality(e);
        ks265_dev_free(main_ctx(e), e->dev_recon);
        if (e->recon_fd >= 0) close(e->recon_fd);
        close_qmaps(e);
    }
    close_lookahead(e); close_input_streams(e);
    close_main(e);
    for (int i = PATH_KEY; i < NPATH; ++i) if (e->path[i].ctx) ks265_destroy(e->path[i].ctx);   /* the contexts: last */
    if (e->ctx_in) ks265_destroy(e->ctx_in);
    if (e->ctx_out) ks265_destroy(e->ctx_out);
    if (e->ctx_rec) ks265_destroy(e->ctx_rec);
    if (main_ctx(e)) ks265_destroy(main_ctx(e));
    close_output(e); close_md5(e);
    pthread_mutex_destroy(&e->la_mu);
    pthread_mutex_destroy(&e->mu); pthread_cond_destroy(&e->cv_work); pthread_cond_destroy(&e->cv_done); pthread_cond_destroy(&e->cv_disp); pthread_cond_destroy(&e->cv_sched); pthread_cond_destroy(&e->cv_sched_done);
    free(e);
}

static Enc *lane_open(QY265EncConfig *cfg, int device, int multi, int *err)
{
    int dummy; if (!err) err = &dummy;
    *err = QY_OK;
    if (!cfg) { *err = QY_POINTER; return NULL; }
    if ((cfg->picWidth & 7) || (cfg->picHeight & 7)) {                  /* a ragged size: even, and the device library has the three entries of picture_window.hip */
        if (cfg->picWidth <= 0 || cfg->picHeight <= 0 || (cfg->picWidth & 1) || (cfg->picHeight & 1) || cfg->picWidth > 8192 || cfg->picHeight > 8192) { *err = QY_NOTSUPPORTED; return NULL; }
        if (!ks265_input_pad || !ks265_input_pad_validate || !ks265_output_crop || !ks265_sse_window) {
            logf_(2, cfg->logLevel, "ks265enc: %dx%d is no multiple of 8 and the device library has no ks265_input_pad\n", cfg->picWidth, cfg->picHeight);
            *err = QY_NOTSUPPORTED; return NULL;
        }
    }
    if (cfg->vpp_denoise || cfg->vpp_recur_filter != 0) {               /* the temporal filter: both fields inside their ranges, and the device library has the two entries */
        if (cfg->vpp_denoise < 0 || cfg->vpp_denoise > 3 || !(cfg->vpp_recur_filter >= 0) || cfg->vpp_recur_filter > 30) { *err = QY_NOTSUPPORTED; return NULL; }
        if (!ks265_input_denoise || !ks265_input_denoise_validate) {
            logf_(2, cfg->logLevel, "ks265enc: vpp_denoise %d / vpp_recur_filter %g asked for and the device library has no ks265_input_denoise\n", cfg->vpp_denoise, cfg->vpp_recur_filter);
            *err = QY_NOTSUPPORTED; return NULL;
        }
    }
    if (cfg->vpp_hdr) {                                                 /* local contrast: 0 / 1, the four values 0 (this build's default) or inside their ranges, and the device library has the entries */
        if (cfg->vpp_hdr != 1 || !(cfg->vpp_hdr_strength >= 0) || cfg->vpp_hdr_strength > 5 || (cfg->vpp_hdr_iter != 0 && cfg->vpp_hdr_iter != 2 && cfg->vpp_hdr_iter != 3) ||
            !(cfg->vpp_hdr_sigma_s >= 0) || cfg->vpp_hdr_sigma_s > 100 || !(cfg->vpp_hdr_sigma_r >= 0) || cfg->vpp_hdr_sigma_r > 100) { *err = QY_NOTSUPPORTED; return NULL; }
        if (!ks265_input_hdr || !ks265_input_hdr_validate || !ks265_input_hdr_work_bytes) {
            logf_(2, cfg->logLevel, "ks265enc: vpp_hdr asked for and the device library has no ks265_input_hdr\n");
            *err = QY_NOTSUPPORTED; return NULL;
        }
    }
    if (cfg->vpp_edge || cfg->vpp_color) {                              /* the enhancement: both fields 0 .. 3, and the device library has the two entries */
        if (cfg->vpp_edge < 0 || cfg->vpp_edge > 3 || cfg->vpp_color < 0 || cfg->vpp_color > 3) { *err = QY_NOTSUPPORTED; return NULL; }
        if (!ks265_input_enhance || !ks265_input_enhance_validate) {
            logf_(2, cfg->logLevel, "ks265enc: vpp_edge %d / vpp_color %d asked for and the device library has no ks265_input_enhance\n", cfg->vpp_edge, cfg->vpp_color);
            *err = QY_NOTSUPPORTED; return NULL;
        }
    }
    if (cfg->picWidth <= 0 || cfg->picHeight <= 0 || (cfg->picWidth & 1) || (cfg->picHeight & 1) || cfg->frameRate <= 0 || cfg->rc < 0 || cfg->rc > 5 || cfg->bframes > GOP_MAX_B) { *err = QY_NOTSUPPORTED; return NULL; }
    Enc *e = (Enc *)calloc(1, sizeof *e);
    if (e) { e->recon_fd = -1; e->qmap_fd = -1; }
    if (!e) { *err = QY_OUTOFMEMORY; return NULL; }
    pthread_mutex_init(&e->la_mu, NULL);
    pthread_mutex_init(&e->mu, NULL); pthread_cond_init(&e->cv_work, NULL); pthread_cond_init(&e->cv_done, NULL); pthread_cond_init(&e->cv_disp, NULL); pthread_cond_init(&e->cv_sched, NULL); pthread_cond_init(&e->cv_sched_done, NULL);
    lane_resolve(e, cfg, device, multi);
    /* The ORDER in which the streams are created matters (round 4, measured at 2160p; DESIGN 6c, tools/hw_queues.hip): a process's normal-priority streams are served by a few
     * in-order hardware queues (four; three where another runtime user - torch in bench.py - holds one) and share them in pairs that depend on the creation order; a stream that
     * shares the pixel path's queue runs in turn with it.  With the lookahead there is a fifth stream: created fourth, in front of the key pictures' stream, it cost 25 % (hierarchical
     * B) / 31 % (IPPP) with not one lookahead kernel launched; created last 8 %; created FIRST nothing measurable - it then pairs with the copy-out stream.  (In the CLI's own
     * process the four normal streams have a queue each; the key pictures' stream is high-priority and has its own.) */
    /* the uploads' stream: created first, like the lookahead's.  Its own even beside the lookahead's: the caller waits for the upload, and behind the analysis kernels of the picture
     * before (measured: 1.17 ms per call instead of the 0.3 ms the DMA takes) it would wait for those too */
    int r = open_early_streams(e);
    if (!r) r = open_main(e);                                          /* the main context, its frame object and the records' layout; with it the ring and the input slots' count (lane_rings) */
    if (!r) r = open_copy_streams(e);
    if (!r) r = open_pipeline(e);
    if (!r) r = open_quality(e);
    if (!r) r = open_qmaps(e);
    if (!r) r = open_dpb(e);
    if (!r) r = open_key_path(e);
    if (!r) r = open_anchor_path(e);
    if (!r) r = open_lookahead(e);                                     /* (the lookahead's objects; its stream was created first - see above) */
    if (!r) r = open_jobs(e);
    if (!r) r = open_inputs(e);
    if (!r) r = open_output(e);
    if (!r) r = open_md5(e);
    if (!r) r = open_devrecon(e);
    if (!r) r = open_threads(e);
    if (!r && e->dn_on) r = ks265_input_denoise_validate(main_ctx(e), &e->dn_cfg, e->W, e->H);
    if (!r && e->en_on) r = ks265_input_enhance_validate(main_ctx(e), &e->en_cfg, e->W, e->H);
    if (!r && e->hdr_on) r = ks265_input_hdr_validate(main_ctx(e), &e->hdr_cfg, e->W, e->H);
    if (r) { *err = hip_rc(r); lane_close(e, 0); return NULL; }
    if (e->en_on) logf_(0, e->log_level, "ks265enc: enhancement on the way in: edge level %d (gain %d/16, core %d, limit %d, over %d), colour level %d (gain %d)\n", cfg->vpp_edge, e->en_cfg.edge_gain,
                        e->en_cfg.edge_core, e->en_cfg.edge_limit, e->en_cfg.edge_over, cfg->vpp_color, e->en_cfg.color_gain);
    if (e->hdr_on) logf_(0, e->log_level, "ks265enc: local contrast on the way in: gain %d/16, %d iterations, slope %d, radii %d / %d / %d (1/16 sample), work buffer %zu bytes\n", e->hdr_cfg.gain,
                         e->hdr_cfg.iters, e->hdr_cfg.slope, e->hdr_cfg.radius[0], e->hdr_cfg.radius[1], e->hdr_cfg.radius[2], e->hdr_bytes);
    if (e->dn_on) logf_(0, e->log_level, "ks265enc: temporal denoiser on the way in: level %d, thr %d, weight %d/32 (motion-compensated, +-8, 16x16 blocks; the history restarts with every GOP chunk a lane is dealt)\n", cfg->vpp_denoise, e->dn_cfg.thr, e->dn_cfg.weight);
    logf_(0, e->log_level, "ks265enc: GPU %d: %dx%d %.2f fps, qp %d, -me %d (hex below %d), subme %d, refs %d, %s, sao %d (%s), key period %d, %d slice writer threads, %s\n", device, e->W, e->H,
          cfg->frameRate, e->base_qp, e->me_method, e->hex_thr, e->subme, e->refs, e->hier ? (e->gop_b == 3 ? "hierarchical-B GOP 4" : "hierarchical-B GOP 8") : e->gop_b ? "P + non-reference B" : "IPPP", e->use_sao,
          e->fcfg.sao == 3 ? "the reference's decision with merge candidates" : e->fcfg.sao == 2 ? "the reference's decision" : e->fcfg.sao ? "the build's rule" : "off", e->iper,
          e->nth, ks265_version());
    return e;
}

static void lane_reconfig(Enc *e, QY265EncConfig *cfg)
{
    if (!e || !cfg) return;
    pthread_mutex_lock(&e->mu);                                        /* lane_put snapshots base_qp / iper into the input slot under this lock */
    e->cfg.qp = cfg->qp; e->cfg.crf = cfg->crf; e->cfg.bitrateInkbps = cfg->bitrateInkbps; e->cfg.iIntraPeriod = cfg->iIntraPeriod;
    e->base_qp = lane_base_qp(cfg, e->cfg.rc); e->iper = cfg->iIntraPeriod;   /* the rate-control mode itself is not reconfigurable: the handle's own rc picks crf / qp */
    pthread_mutex_unlock(&e->mu);
}
static int lane_headers(Enc *e, QY265Nal **pNals, int *n)
{
    if (!e || !pNals || !n) return QY_POINTER;
    long off = 0;                                                       /* VPS, SPS, PPS as three entries (as in front of a key picture): callers build hvcC / extradata per entry */
    for (int k = 0; k < 3; ++k) {
        e->nals[k].naltype = KS265_NAL_VPS + k; e->nals[k].tid = 0; e->nals[k].iSize = (int)e->hdr_part[k]; e->nals[k].pts = 0; e->nals[k].pPayload = e->hdr + off;
        off += e->hdr_part[k];
    }
    *pNals = e->nals; *n = 3;
    return QY_OK;
}
static int lane_delayed(Enc *e)
{
    if (!e) return 0;
    int n = 0;
    pthread_mutex_lock(&e->mu);                                        /* one snapshot: a picture moves from "waiting" to "in flight" under this lock */
    for (int i = 0; i < MAX_INPUT; ++i) if (e->in[i].used == IN_READY) ++n;
    n += e->njobs + e->la_qn;                                          /* (la_q: at the input, their analysis still running) */
    pthread_mutex_unlock(&e->mu);
    return n;
}

/* zero-copy input: hand the caller one of the lane's pinned input slots to write the next picture into; QY265EncoderEncodeFrame recognises the
 * pointer and copies nothing.  Never blocks: QY_FAIL when no slot is free right now (the caller then passes its own buffer, which is copied as usual). */
static int lane_acquire(Enc *e, QY265YUV *yuv)
{
    Input *slot = NULL;
    pthread_mutex_lock(&e->mu);
    for (int i = 0; i < e->nin && !slot; ++i) if (e->in[i].used == IN_ACQUIRED) slot = &e->in[i];
    for (int i = 0; i < e->nin && !slot; ++i) if (e->in[i].used == IN_FREE) slot = &e->in[i];
    if (slot) slot->used = IN_ACQUIRED;
    pthread_mutex_unlock(&e->mu);
    if (!slot) return QY_FAIL;
    yuv->iWidth = e->srcW; yuv->iHeight = e->srcH;                     /* (the caller's size: the coded one unless the lane is ragged) */
    yuv->pData[0] = slot->i420; yuv->pData[1] = slot->i420 + (size_t)e->srcW * e->srcH; yuv->pData[2] = yuv->pData[1] + (size_t)e->srcW * e->srcH / 4;
    yuv->iStride[0] = e->srcW; yuv->iStride[1] = e->srcW / 2; yuv->iStride[2] = e->srcW / 2;
    return QY_OK;
}

/* ---- the lookahead at the input (-lookahead N, or by itself with the SDK's default GOP).  Round 4: nobody waits for it.  A picture's analysis is launched on a stream of its own
 *      when the picture is handed in; the picture then sits in a short queue (la_q, display order) until its results have arrived - looked at, not waited for, whenever the caller
 *      hands in another picture - and only then goes to the scheduler.  The queue holds at most LA_KEEP pictures: a result that is still missing then is waited for (the analysis
 *      has had several picture times by then).  Same decisions as when the caller waited for every picture (round 3; the CPU tests did not change), a few pictures of delay at
 *      the input.  The caller's thread launches; the caller's thread and - when it has nothing to schedule - the scheduler thread look (la_mu). */
#define LA_KEEP (e->la_keep)

/* a picture whose analysis is through (or which needs none) goes to the scheduler */
static void la_publish(Enc *e, Input *slot, int cut, int mini4)
{
    const int nd = slot->disp;
    pthread_mutex_lock(&e->mu);
    if (!e->la_auto) {                                                 /* (auto: no scene cuts, the key positions are known when the picture is handed in - la_take keeps them) */
        const int periodic = slot->iper > 0 && e->la_last_key > NO_PIC && nd - e->la_last_key >= slot->iper;    /* (the scheduler's own rule: key positions are the same there) */
        if (cut) ++e->la_cuts;
        if (cut || slot->key || nd == 0 || periodic) e->la_last_key = nd;
    }
    slot->mini4 = mini4; slot->key = slot->key || cut; slot->used = IN_READY; e->next_disp = nd + 1;
    pthread_cond_signal(&e->cv_sched);
    pthread_mutex_unlock(&e->mu);
}

/* the results of one analysed picture: the scene-cut verdict and, with the hierarchical GOP, the slice types of its block of 8 */
static void la_decide(Enc *e, const Input *slot, int *cut_out, int *mini4_out)
{
    const int nd = slot->disp, w = e->la_w, h = e->la_h;
    const uint64_t *out = e->la_host_out + 16 * slot->la_buf;
    int cut = 0, mini4 = 0;
    if (slot->la_what & 1) {                                           /* scene cut: the picture against its predecessor */
        /* a cut: predicting the picture from its predecessor costs at least 0.7 of coding it intra (both sums over the 8x8 blocks of the half-size picture),
         * and the last key picture is at least eight pictures back */
        if (g_cli.scenecut > 0) {
            /* -scenecut N: the reference's verdict (scenecut enc@0x47e9d0, restated in oracle/ks265_lookahead_ref.c and pinned on recorded calls) on this lookahead's
             * frame costs: a change of flatness (intra cost below 4 per 8x8 block of the half-size picture) decides at once; else a cut is where predicting the
             * picture costs at least (1 - N / 100 x pictures since the key picture / min(key period, 320)) of coding it intra */
            const long long icost = (long long)out[0], pcost = (long long)out[1], prev = e->la_prev_icost;
            const long long T = (long long)(w / 8) * (h / 8) * 4;
            int verdict = -1;
            if (prev >= 0) {
                if (prev < T) { if (icost > T) verdict = 1; else if (icost < T) verdict = 0; }
                else if (prev > T && icost < T) verdict = 1;
            }
            if (verdict < 0) {
                const int keyint = slot->iper > 0 ? (slot->iper < 320 ? slot->iper : 320) : 256;
                const double bias = (double)(nd - (e->la_last_key > NO_PIC ? e->la_last_key : 0)) * ((double)g_cli.scenecut / 100.0) / (double)keyint;
                verdict = (double)pcost >= (1.0 - bias) * (double)icost;
            }
            cut = verdict;
            e->la_prev_icost = icost;
        } else if (out[1] * 10 >= out[0] * 7 && nd - e->la_last_key >= 8) cut = 1;
    }
    /* slice types of the hierarchical GOP (the reference's adaptive BiPredFrames): the GOP is laid out in blocks of 8 pictures from its key picture; a block is
     * coded with its anchor 8 pictures after the previous one, or - when predicting that anchor from 8 pictures back costs more than the two anchors 4 apart cost
     * together (+ 1/12: the shorter structure pays more B-picture overhead) - as two mini-GOPs of 4.  Costs = the inter sums of the frame-cost kernels, this
     * picture against the pictures 4 and 8 back; decided at the block's last picture, carried to the scheduler in its input slot. */
    if ((slot->la_what & 2) && !cut) {                                 /* (launched before the verdict was known: a cut starts a GOP here, the grid's sums are not used) */
        const int p = slot->la_p;
        const unsigned long long c4 = out[5];
        if ((p & 7) == 0) {
            const unsigned long long c8 = out[9], two = c4 + e->la_c4_prev;
            mini4 = c8 * 12 > two * 13;
            if (mini4) ++e->la_mini4;
        }
        e->la_c4_prev = c4;
    }
    *cut_out = cut; *mini4_out = mini4;
}

/* hand the queue's pictures to the scheduler, oldest first, as far as their results are there; while more than `keep` pictures are queued the oldest one's results are waited for */
static int la_drain_locked(Enc *e, int keep)
{
    while (e->la_qn > 0) {
        Input *h = e->la_q[0];
        int cut = 0, mini4 = 0;
        if (h->la_what >= 0) {
            int r, done = 1;
            if (e->la_qn > keep) { const double t0 = now_ms(); r = ks265_event_wait(e->ctx_la, e->la_evs[h->la_buf]); e->la_t_wait += now_ms() - t0; ++e->la_n_wait; }
            else r = ks265_event_query(e->ctx_la, e->la_evs[h->la_buf], &done);
            if (r) { pthread_mutex_lock(&e->mu); for (int i = 0; i < e->la_qn; ++i) e->la_q[i]->used = IN_FREE; e->la_qn = 0; e->la_flying = 0; e->sched_err = hip_rc(r); pthread_mutex_unlock(&e->mu); return hip_rc(r); }
            if (!done) break;
            la_decide(e, h, &cut, &mini4);
            --e->la_flying;
        }
        la_publish(e, h, cut, mini4);
        memmove(e->la_q, e->la_q + 1, sizeof e->la_q[0] * (size_t)(e->la_qn - 1));
        __atomic_store_n(&e->la_qn, e->la_qn - 1, __ATOMIC_RELEASE);
    }
    return QY_OK;
}
static int la_drain(Enc *e, int keep)
{
    pthread_mutex_lock(&e->la_mu);
    const int r = la_drain_locked(e, keep);
    pthread_mutex_unlock(&e->la_mu);
    return r;
}

/* a picture handed in: its half-size picture and the frame-cost kernels it needs (against its predecessor: scene cut; on the GOP's grid of 4 against the pictures 4 and 8
 * back: slice types), results on their way to the host; into the queue */
static int la_take_locked(Enc *e, Input *slot)
{
    int r;
    /* -lookahead N: a scene-cut verdict moves the GOP's grid, so the next picture's launch needs every verdict before it; auto: nothing of the launch depends on results.
     * At most four analyses in flight (their result areas) */
    if ((r = la_drain_locked(e, e->la_auto ? LA_KEEP : 0))) return r;
    while (e->la_flying >= LA_FLY || e->la_qn >= LA_QMAX - 1) if ((r = la_drain_locked(e, e->la_qn - 1))) return r;
    const int nd = slot->disp, c = nd % LA_RING, w = e->la_w, h = e->la_h;
    const size_t org = (size_t)e->geom_la.pad_y * e->geom_la.stride_y + e->geom_la.pad_y;
    const int keynow = slot->key || nd == 0 || (slot->iper > 0 && e->la_last_key > NO_PIC && nd - e->la_last_key >= slot->iper);   /* (but for a scene cut, not known yet) */
    const int p = keynow ? 0 : nd - e->la_last_key;                    /* position inside the GOP */
    if (e->la_auto && keynow) e->la_last_key = nd;
    int what = -1;
    r = 0;
    if (!e->la_auto || (p & 3) == 0) {                                 /* auto: pictures off the grid are neither analysed nor kept */
        const int buf = e->la_seq++ % LA_FLY;
        uint64_t *dout = e->la_dev_out + 16 * buf;
        what = 0;
        /* the half-size picture from the slot's twin on the device (uploaded a moment ago on this stream).  Measured in round 4 before that existed: an H2D copy of the
         * luma plane on this stream (round 3) queues on the copy engine BEHIND the uploads the scheduler had enqueued, which waited for the pipeline's buffers - the results
         * arrived 10 ms and more late; kernels reading the pinned picture over PCIe instead (ks265_downsample_from_host, 64 work-groups) cost the encoder 28 % */
        r = e->ctx_up != e->ctx_la && !slot->up_sync ? ks265_stream_wait_event(e->ctx_la, slot->ev_up) : 0;      /* (the upload runs on a stream of its own) */
        if (!r) r = ks265_downsample_rect(e->ctx_la, slot->dev, e->W, e->la_pic[c].y + org, e->geom_la.stride_y, w, h);
        if (!r) r = ks265_pad_picture(e->frame_la, e->la_pic[c]);
        if (!r && e->la_have_prev && !e->la_auto) {
            r = ks265_lookahead_picture(e->frame_la, e->la_pic[c], e->la_pic[(nd + LA_RING - 1) % LA_RING], e->la_cost_ws, dout);
            what |= 1;
        }
        if (!r && e->mg_adapt && p >= 4 && (p & 3) == 0) {
            /* (-lookahead N: the picture's intra costs are in la_cost_ws from the call above - search + sums only; auto: NO intra pass since round 5 - the slice-type decision
             *  reads the searches' sums alone (la_decide: out[5], out[9]), and the pass was 0.3 ms per grid picture = 6 % of the device's time with the default GOP) */
            const uint32_t *ws = e->la_auto ? NULL : e->la_cost_ws;
            r = ks265_lookahead_inter(e->frame_la, e->la_pic[c], e->la_pic[(nd - 4) % LA_RING], ws, dout + 4);
            if (!r && (p & 7) == 0) r = ks265_lookahead_inter(e->frame_la, e->la_pic[c], e->la_pic[(nd - 8) % LA_RING], ws, dout + 8);
            what |= 2;
        }
        if (!r && what) r = ks265_memcpy_d2h_async(e->ctx_la, e->la_host_out + 16 * buf, dout, 96);
        if (!r) r = ks265_event_record(e->ctx_la, e->la_evs[buf]);     /* (the slot's pinned picture is being read by the upload: the slot stays here until the event has passed) */
        if (r) return hip_rc(r);
        e->la_have_prev = 1; slot->la_buf = buf; ++e->la_flying;
    }
    slot->la_what = what; slot->la_p = p;
    e->la_q[e->la_qn] = slot;
    __atomic_store_n(&e->la_qn, e->la_qn + 1, __ATOMIC_RELEASE);
    return la_drain_locked(e, LA_KEEP);
}
static int la_take(Enc *e, Input *slot)
{
    pthread_mutex_lock(&e->la_mu);
    const int r = la_take_locked(e, slot);
    pthread_mutex_unlock(&e->la_mu);
    return r;
}

/* ---- the application's picture buffers, pinned in place once and remembered (process-wide: hipHostRegister refuses memory that is registered already) --------------------------- */
#define REG_MAX 160
static struct { pthread_mutex_t mu; struct { uint8_t *base; size_t n; unsigned long stamp; } ent[REG_MAX]; int n; unsigned long clock; uint8_t *bad[32]; int nbad; int handles; } g_reg = {.mu = PTHREAD_MUTEX_INITIALIZER};
static int reg_get(ks265_ctx *c, uint8_t *p, size_t n, int may_evict)
{
    int ok = 0;
    pthread_mutex_lock(&g_reg.mu);
    ++g_reg.clock;
    for (int i = 0; i < g_reg.n && !ok; ++i)
        if (p >= g_reg.ent[i].base && p + n <= g_reg.ent[i].base + g_reg.ent[i].n) { g_reg.ent[i].stamp = g_reg.clock; ok = 1; }
    for (int i = 0; i < g_reg.nbad && !ok; ++i) if (g_reg.bad[i] == p) { pthread_mutex_unlock(&g_reg.mu); return 0; }
    if (!ok) {
        for (int i = 0; i < g_reg.n; )                                 /* a buffer that overlaps an older registration: that memory has been given back and handed out again */
            if (p < g_reg.ent[i].base + g_reg.ent[i].n && g_reg.ent[i].base < p + n) { (void)ks265_host_unregister(c, g_reg.ent[i].base); g_reg.ent[i] = g_reg.ent[--g_reg.n]; } else ++i;
        if (g_reg.n == REG_MAX && may_evict) {                         /* least recently used */
            int lru = 0;
            for (int i = 1; i < g_reg.n; ++i) if (g_reg.ent[i].stamp < g_reg.ent[lru].stamp) lru = i;
            (void)ks265_host_unregister(c, g_reg.ent[lru].base); g_reg.ent[lru] = g_reg.ent[--g_reg.n];
        }
        if (g_reg.n < REG_MAX && ks265_host_register(c, p, n) == KS265_OK) { g_reg.ent[g_reg.n].base = p; g_reg.ent[g_reg.n].n = n; g_reg.ent[g_reg.n++].stamp = g_reg.clock; ok = 1; }
        else if (g_reg.nbad < 32) g_reg.bad[g_reg.nbad++] = p;         /* memory the runtime cannot pin: that buffer is copied from now on */
    }
    pthread_mutex_unlock(&g_reg.mu);
    return ok;
}
static void reg_handle(ks265_ctx *c, int open)
{
    pthread_mutex_lock(&g_reg.mu);
    g_reg.handles += open ? 1 : -1;
    if (!open && g_reg.handles == 0) { for (int i = 0; i < g_reg.n; ++i) (void)ks265_host_unregister(c, g_reg.ent[i].base); g_reg.n = 0; g_reg.nbad = 0; }   /* the last lane of the process lets go of the application's memory */
    pthread_mutex_unlock(&g_reg.mu);
}

/* the conversion's view of a device picture of the lane's size */
static void dev_desc(const Enc *e, const ks265_dev_picture *p, ks265_in_desc *d)
{
    *d = (ks265_in_desc){.format = p->format, .width = e->srcW, .height = e->srcH, .pixel_step = p->pixel_step, .matrix = p->matrix, .full_range = p->full_range};   /* (the caller's size: the coded one unless the lane is ragged) */
    for (int k = 0; k < 3; ++k) { d->plane[k] = p->plane[k]; d->pitch[k] = p->pitch[k]; }
}

/* a ragged lane: the picture that lies (or, on ctx_up, is on its way) in the slot's staging area becomes the slot's twin of the coded size, and ev_up is recorded behind that */
static int lane_pad_slot(Enc *e, Input *slot)
{
    const size_t ny = (size_t)e->srcW * e->srcH;
    const ks265_in_desc d = {.format = KS265_IN_I420, .width = e->srcW, .height = e->srcH, .plane = {slot->raw, slot->raw + ny, slot->raw + ny + ny / 4}, .pitch = {e->srcW, e->srcW / 2, e->srcW / 2}};
    const int r = ks265_input_pad(e->ctx_up, &d, e->W, e->H, slot->dev);
    return r ? r : ks265_event_record(e->ctx_up, slot->ev_up);
}

/* the picture being handed in, filled once by the API entry (QY265EncoderEncodeFrame, resolve_device) and passed down as it is: top_encode adds the pending ROI map, lane_put
 * runs what `how` says and decides nothing again.  how: a host picture (yuv); a device picture (dp, validated; d: the operation's view of it) converted / padded (a ragged lane) /
 * scaled (d at the source's size; sc: kept by the lane this picture goes to, any context of the device may run it) into the slot's twin.  roi: the pending map or NULL */
enum { PIC_HOST, PIC_CONVERT, PIC_PAD, PIC_SCALE };
/* the overlays in force for one picture (top_encode: the handle's slots in ascending number, without the forced-only ones unless the call forced them), as the device
 * library takes them, and the caller's streams the device overlays among them are read in the order of (each once; nst = 0: host overlays only) */
typedef struct OvSet { int n, nst; ks265_overlay_desc d[KS265_OV_SLOTS]; void *stream[KS265_OV_SLOTS]; } OvSet;
typedef struct PicIn { int how; long long pts; const QY265YUV *yuv; const ks265_dev_picture *dp; ks265_in_desc d; const struct ScalePlan *sc; const ks265_roi *roi;
                       int tm;                            /* a device picture that is tone-mapped (ks265_enc_enable_tonemap) where it would be converted; scaled: in front of the scaler */
                       int force_logo; const OvSet *ovs; /* bForceLogo of the call; the overlays or NULL (top_encode) */ } PicIn;
/* back-pressure on the input side (mu held): at most 16 pictures wait for the scheduler thread (it may itself be waiting for ring space, which only the caller's take_output
 * frees - then go on and collect).  GOP lanes (multi): the input slots are the limit (lane_has_slot) - a lane takes a whole GOP in while it is still coding the previous one, or
 * the caller would wait here while the other lanes run dry.  cuTree: the scheduler itself holds a mini-GOP back until its window has arrived - that many more may wait */
static void wait_input_room(Enc *e, double since)
{
    while (!e->multi && !e->quit && !e->sched_err && e->next_disp - (e->coded_upto + 1) > 16 + (e->ct_on ? e->ct_depth + e->gop_b + 1 : 0) && e->njobs <= e->ring - 12) pthread_cond_wait(&e->cv_sched_done, &e->mu);
    e->la_t_bp += now_ms() - since;                                    /* (a scheduler that failed makes no more progress) */
}
/* the slot the picture goes into (mu held), IN_FILLING from here; *own: the caller wrote the picture into this slot after acquiring it (ks265_enc_acquire_input): nothing to copy.
 * NULL - one lane: cannot happen (more input slots than pictures in flight + one mini-GOP); lanes: the caller checked lane_has_slot */
static Input *take_input_slot(Enc *e, const uint8_t *data, int *own)
{
    Input *slot = NULL; *own = 0;
    for (int i = 0; i < e->nin && !slot && data; ++i) if (e->in[i].used == IN_ACQUIRED && e->in[i].i420 == data) { slot = &e->in[i]; *own = 1; }
    for (int i = 0; i < e->nin && !slot; ++i) if (e->in[i].used == IN_FREE) slot = &e->in[i];
    for (int i = 0; i < e->nin && !slot; ++i) if (e->in[i].used == IN_ACQUIRED) slot = &e->in[i];   /* last resort: the caller's pointer to it is dead from here on, as after any EncodeFrame call */
    if (slot) { slot->used = IN_FILLING; slot->up_sync = 0; slot->roi_has = 0; }
    return slot;
}
/* the bracket around work on ctx_up that reads memory of a stream of the caller's: that stream -> ctx_up (in), the work, then its event and the caller's stream waits for it (out) */
static int caller_stream_in(Enc *e, void *stream) { return ks265_wait_external(e->ctx_up, stream); }
static int caller_stream_out(Enc *e, void *stream, void *ev) { const int r = ks265_event_record(e->ctx_up, ev); return r ? r : ks265_external_wait_event(e->ctx_up, stream, ev); }
/* the map becomes the slot's record on ctx_up, beside the picture's own way in.  A map describes the caller's picture; the CTU grid is the coded picture's */
static int stage_roi(Enc *e, Input *slot, const ks265_roi *roi)
{
    const int sw = e->srcW, sh = e->srcH; int r;
    if (roi->device >= 0) {
        const ks265_roi_desc d = {roi->type, roi->log2_block, ks265_roi_map_cols(sw, roi->log2_block), ks265_roi_map_rows(sh, roi->log2_block), roi->data, roi->pitch};
        r = caller_stream_in(e, roi->stream);
        if (!r) r = ks265_roi_reduce(e->ctx_up, &d, sw, sh, slot->roi_rec);
        if (!r) r = caller_stream_out(e, roi->stream, slot->ev_roi);
    } else {                                                           /* host memory: reduced here, on the calling thread (ks265_roi.h); the record is uploaded */
        r = ks265_roi_reduce_host(roi->type, roi->log2_block, roi->data, roi->pitch, sw, sh, slot->roi_host) ? KS265_NOTSUPPORTED : KS265_OK;
        if (!r) r = ks265_memcpy_h2d_async(e->ctx_up, slot->roi_rec, slot->roi_host, (size_t)e->geom.ctu_cols * e->geom.ctu_rows * sizeof(int32_t));
        if (!r) r = ks265_event_record(e->ctx_up, slot->ev_roi);
    }
    if (!r) slot->roi_has = 1;
    return r;
}
/* a device picture: the resolved operation into the twin, in the order of the caller's stream (a scaled one in the same place between the same two events) */
static int stage_device(Enc *e, Input *slot, const PicIn *p)
{
    int r = caller_stream_in(e, p->dp->stream);
    if (!r && p->tm) {                                                 /* tone-mapped at its own size: into the twin, or into the scaler's way-station picture and scaled from there as I420 */
        const size_t sn = (size_t)p->d.width * p->d.height;
        const ks265_in_desc sdr = {.format = KS265_IN_I420, .width = p->d.width, .height = p->d.height, .plane = {e->sc_scratch, e->sc_scratch + sn, e->sc_scratch + sn + sn / 4}, .pitch = {p->d.width, p->d.width / 2, p->d.width / 2}};
        r = ks265_input_tonemap(e->ctx_up, e->tm_plan, &p->d, p->how == PIC_SCALE ? e->sc_scratch : slot->dev);
        if (!r && p->how == PIC_SCALE) r = ks265_input_scale(e->ctx_up, p->sc->plan, &sdr, NULL, slot->dev);
        return r ? r : caller_stream_out(e, p->dp->stream, slot->ev_up);
    }
    if (!r) r = p->how == PIC_SCALE ? ks265_input_scale(e->ctx_up, p->sc->plan, &p->d, e->sc_scratch, slot->dev)
              : p->how == PIC_PAD ? ks265_input_pad(e->ctx_up, &p->d, e->W, e->H, slot->dev) : ks265_input_convert(e->ctx_up, &p->d, slot->dev);
    return r ? r : caller_stream_out(e, p->dp->stream, slot->ev_up);
}
static uint8_t *upload_dst(const Enc *e, const Input *slot) { return e->ragged ? slot->raw : slot->dev; }   /* a ragged lane's staging area: ks265_input_pad behind it (lane_pad_slot) */
static int packed_strides(const Enc *e, const QY265YUV *yuv) { return yuv->iStride[0] == e->srcW && yuv->iStride[1] == e->srcW / 2 && yuv->iStride[2] == e->srcW / 2; }
/* packed planes that the runtime can pin where they lie go up from there, whole or plane by plane - *took (else nothing has happened: the picture is copied).  direct_in 2: no stream, the call returns when the
 * picture is on the device (a ragged lane's twin is still made on ctx_up: its readers wait for ev_up as after any other upload); 1: on ctx_up, waited for at the end of the API call (finish_upload) */
static int stage_host_direct(Enc *e, Input *slot, const QY265YUV *yuv, int *took)
{
    const size_t ny = (size_t)e->srcW * e->srcH, nc = ny / 4;
    uint8_t *const up = upload_dst(e, slot);
    const int whole = yuv->pData[1] == yuv->pData[0] + ny && yuv->pData[2] == yuv->pData[1] + nc, np = whole ? 1 : 3, sync = e->direct_in == 2;
    const struct { uint8_t *dst, *src; size_t n; } piece[3] = {{up, yuv->pData[0], whole ? ny + 2 * nc : ny}, {up + ny, yuv->pData[1], nc}, {up + ny + nc, yuv->pData[2], nc}};
    for (int k = 0; k < np; ++k) if (!reg_get(e->ctx_up, piece[k].src, piece[k].n, !e->hold_in)) return KS265_OK;   /* (hold: an old registration may still be read by a DMA in flight - then the table only grows) */
    int r = KS265_OK; *took = 1;
    for (int k = 0; k < np && !r; ++k) r = sync ? ks265_memcpy_h2d_sync(main_ctx(e), piece[k].dst, piece[k].src, piece[k].n) : ks265_memcpy_h2d_async(e->ctx_up, piece[k].dst, piece[k].src, piece[k].n);
    if (sync && !e->ragged) slot->up_sync = 1;
    else if (!r) r = e->ragged ? lane_pad_slot(e, slot) : ks265_event_record(e->ctx_up, slot->ev_up);
    if (!sync && !e->hold_in) e->pending_up = slot;
    return r;
}
/* into the slot's pinned memory (own: it lies there) - packed planes as three block copies, else row by row - and from there to the device at once, on the lookahead's stream
 * (nothing there waits for the pipeline) */
static int stage_host_copy(Enc *e, Input *slot, const QY265YUV *yuv, int own)
{
    const int sw = e->srcW, sh = e->srcH;
    uint8_t *u = slot->i420 + (size_t)sw * sh, *v = u + (size_t)sw * sh / 4;
    if (!own && packed_strides(e, yuv)) {
        copy_shared(e->pool, slot->i420, yuv->pData[0], (size_t)sw * sh);
        copy_shared(e->pool, u, yuv->pData[1], (size_t)sw * sh / 4);
        copy_shared(e->pool, v, yuv->pData[2], (size_t)sw * sh / 4);
    } else if (!own) {
        for (int y = 0; y < sh; ++y) memcpy(slot->i420 + (size_t)y * sw, yuv->pData[0] + (size_t)y * yuv->iStride[0], (size_t)sw);
        for (int y = 0; y < sh / 2; ++y) {
            memcpy(u + (size_t)y * (sw / 2), yuv->pData[1] + (size_t)y * yuv->iStride[1], (size_t)sw / 2);
            memcpy(v + (size_t)y * (sw / 2), yuv->pData[2] + (size_t)y * yuv->iStride[2], (size_t)sw / 2);
        }
    }
    if (!slot->dev) return KS265_OK;
    const int r = ks265_memcpy_h2d_async(e->ctx_up, upload_dst(e, slot), slot->i420, (size_t)sw * sh * 3 / 2);
    return r ? r : e->ragged ? lane_pad_slot(e, slot) : ks265_event_record(e->ctx_up, slot->ev_up);
}
/* `vpp_denoise`: the slot's twin, whichever way it was made, is filtered in place on ctx_up against the lane's last filtered picture, and ev_up is recorded again behind that:
 * a host-synchronous upload has finished by now, but its readers must wait for the filter (up_sync off).  key: a GOP chunk starts on this lane - no history, like the lane's
 * first picture (one lane: key is never set here, the recursion runs across the periodic key pictures) */
static int stage_denoise(Enc *e, Input *slot, int key)
{
    const int to = e->dn_has ? e->dn_at ^ 1 : 0;
    int r = ks265_input_denoise(e->ctx_up, &e->dn_cfg, e->W, e->H, slot->dev, e->dn_has && !key ? e->dn_hist[e->dn_at] : NULL, e->dn_hist[to], NULL);
    if (!r) r = ks265_event_record(e->ctx_up, slot->ev_up);
    slot->up_sync = 0; e->dn_at = to; e->dn_has = 1;
    return r;
}
/* `vpp_hdr`: the luma of the slot's twin gets its local contrast raised in place on ctx_up, behind the denoiser - whose history pictures stay as they are: the recursion never
 * sees boosted samples - and in front of the enhancement (sharpening comes last); ev_up is recorded again behind it (up_sync off, as behind its neighbours) */
static int stage_hdr(Enc *e, Input *slot)
{
    int r = ks265_input_hdr(e->ctx_up, &e->hdr_cfg, e->W, e->H, slot->dev, e->hdr_work, e->hdr_bytes);
    if (!r) r = ks265_event_record(e->ctx_up, slot->ev_up);
    slot->up_sync = 0;
    return r;
}
/* `vpp_edge` / `vpp_color`: the slot's twin is enhanced on ctx_up, the last step in front of the encoder, and ev_up is recorded again behind it (up_sync off, as behind the
 * denoiser).  The luma stencil reads a copy: the history picture the denoiser has just written (dn_hist[dn_at] - the twin's bytes; it stays unsharpened, the recursion never
 * sees enhanced samples), else - without the denoiser, or with `vpp_hdr` between the two - the lane's own plane, copied in front of the launch.  vpp_color alone needs none */
static int stage_enhance(Enc *e, Input *slot)
{
    const uint8_t *luma = NULL;
    int r = KS265_OK;
    if (e->en_cfg.edge_gain) {
        if (e->dn_on && !e->hdr_on) luma = e->dn_hist[e->dn_at];
        else { r = ks265_memcpy_d2d_async(e->ctx_up, e->en_luma, slot->dev, (size_t)e->W * e->H); luma = e->en_luma; }
    }
    if (!r) r = ks265_input_enhance(e->ctx_up, &e->en_cfg, e->W, e->H, luma, slot->dev);
    if (!r) r = ks265_event_record(e->ctx_up, slot->ev_up);
    slot->up_sync = 0;
    return r;
}
/* overlays (ks265_enc_set_overlay): the picture's set is blended onto the slot's twin by one launch on ctx_up, the last step in front of the encoder - behind the filters, so
 * neither they nor the denoiser's history ever see it - inside the bracket of every caller's stream a device overlay is read in the order of, and ev_up is recorded again
 * behind it (up_sync off, as behind its neighbours).  The window is the caller's picture: a ragged lane's padding keeps its bytes */
static int stage_overlay(Enc *e, Input *slot, const OvSet *ovs)
{
    int r = KS265_OK;
    for (int k = 0; k < ovs->nst && !r; ++k) r = caller_stream_in(e, ovs->stream[k]);
    if (!r) r = ks265_input_overlay(e->ctx_up, ovs->d, ovs->n, e->W, e->H, e->srcW, e->srcH, slot->dev);
    if (!r) r = ks265_event_record(e->ctx_up, slot->ev_up);
    for (int k = 0; k < ovs->nst && !r; ++k) r = ks265_external_wait_event(e->ctx_up, ovs->stream[k], slot->ev_up);
    slot->up_sync = 0;
    return r;
}
/* the picture's own fields travel with it from now, and it goes on to the scheduler thread - at once, or with the lookahead when its results are there (la_drain).  A QY code */
static int publish_input(Enc *e, Input *slot, long long pts, int key)
{
    pthread_mutex_lock(&e->mu);
    slot->mini4 = 0; slot->disp = e->in_disp++; slot->pts = pts; slot->key = key || e->force_key; slot->base_qp = e->base_qp; slot->iper = e->iper; slot->kbps = e->cfg.bitrateInkbps;
    e->force_key = 0;
    if (!e->la_on) { slot->used = IN_READY; e->next_disp = e->in_disp; pthread_cond_signal(&e->cv_sched); }
    pthread_mutex_unlock(&e->mu);
    if (!e->la_on) return QY_OK;
    const double t0 = now_ms();
    const int r = la_take(e, slot);
    e->la_t_take += now_ms() - t0;
    return r;
}
/* the one way out of a failed way in: the slot is free again and the lane has failed */
static int input_fail(Enc *e, Input *slot, int rc) { pthread_mutex_lock(&e->mu); slot->used = IN_FREE; e->sched_err = rc; pthread_mutex_unlock(&e->mu); return rc; }
/* one picture into the lane and on to the scheduler thread.  key: it starts a closed GOP regardless of the period */
static int lane_put(Enc *e, const PicIn *p, int key)
{
    const QY265YUV *yuv = p->yuv;
    if (p->how == PIC_HOST && (!yuv || !yuv->pData[0] || !yuv->pData[1] || !yuv->pData[2])) return QY_POINTER;
    if (p->how == PIC_HOST && (yuv->iWidth != e->srcW || yuv->iHeight != e->srcH)) return QY_NOTSUPPORTED;
    const double tc0 = now_ms();
    int own, direct = 0;
    pthread_mutex_lock(&e->mu);
    wait_input_room(e, tc0);
    Input *slot = take_input_slot(e, p->how == PIC_HOST ? yuv->pData[0] : NULL, &own);
    pthread_mutex_unlock(&e->mu);
    if (!slot) return QY_FAIL;
    int r = p->roi && e->roi_on ? stage_roi(e, slot, p->roi) : KS265_OK;
    if (!r && p->how != PIC_HOST) r = stage_device(e, slot, p);
    if (!r && p->how == PIC_HOST && e->direct_in && !own && slot->dev && packed_strides(e, yuv)) r = stage_host_direct(e, slot, yuv, &direct);
    if (!r && p->how == PIC_HOST && !direct) r = stage_host_copy(e, slot, yuv, own);
    if (!r && e->dn_on) r = stage_denoise(e, slot, key);
    if (!r && e->hdr_on) r = stage_hdr(e, slot);
    if (!r && e->en_on) r = stage_enhance(e, slot);
    if (!r && p->ovs) r = stage_overlay(e, slot, p->ovs);
    if (r) { e->pending_up = NULL; r = hip_rc(r); }                    /* (nothing of a failed picture is waited for) */
    else r = publish_input(e, slot, p->pts, key);
    if (r) return input_fail(e, slot, r);
    e->st.in_copy_ms += now_ms() - tc0;
    return QY_OK;
}

/* the caller's buffer is its own again when the API call returns: the upload out of it (stage_host_direct on ctx_up) has finished.  A QY code */
static int finish_upload(Enc *e)
{
    if (!e->pending_up) return QY_OK;
    const double tw = now_ms();
    const int ru = ks265_event_wait(e->ctx_up, e->pending_up->ev_up);
    e->pending_up = NULL; e->st.in_copy_ms += now_ms() - tw;
    return hip_rc(ru);
}
/* flush, first half: everything that has arrived gets scheduled (short mini-GOPs at the end).  Returns 1 when the scheduler is through, 0 when the ring
 * filled up first (the scheduler then waits for the caller to collect output: hand out what is ready and come back, as the SDK's flush loop does anyway -
 * EncodeFrame(NULL) while DelayedFrames() > 0) */
static int lane_flush_begin(Enc *e, int wait)
{
    if (e->la_on) (void)la_drain(e, 0);                                /* the pictures whose analysis is still running: waited for (an error is in sched_err) */
    pthread_mutex_lock(&e->mu);
    e->sched_flush = 1;
    pthread_cond_signal(&e->cv_sched);
    int all = 0;
    for (;;) {
        all = !e->sched_flush && e->sched_idle && e->sched_seen == e->next_disp;
        if (all || !wait || e->quit || e->njobs > e->ring - 12) break;   /* GOP lanes do not wait here: while the caller sat in one lane's flush nobody would collect from the others */
        pthread_cond_wait(&e->cv_sched_done, &e->mu);
    }
    pthread_mutex_unlock(&e->mu);
    return all;
}

static int lane_encode_frame(Enc *e, QY265Nal **pNals, int *iNalCount, const PicIn *p, QY265Picture *out)
{
    *pNals = e->nals; *iNalCount = 0;
    int r = QY_OK;
    if (p) {
        r = lane_put(e, p, 0);
        if (r) return r;
        /* finished pictures (copied to the output buffer); when the ring of in-flight pictures is nearly full, wait for the oldest ones -
         * only as many as needed, the writers keep running */
        const double t0 = now_ms();
        int in_flight = e->ring - 12;
        if (e->zero_latency) {
            /* -latency zerolatency (QY265LATENCY_ZERO; the SDK's live-streaming mode): the call returns with THIS picture's NAL units - nothing stays behind, QY265EncoderDelayedFrames
             * is 0 between calls.  The picture goes through the same pipeline (scheduler thread, streams, writer threads sharing its rows); the caller waits for it */
            pthread_mutex_lock(&e->mu);
            while (!e->quit && !e->sched_err && (e->sched_seen != e->next_disp || !e->sched_idle)) pthread_cond_wait(&e->cv_sched_done, &e->mu);
            pthread_mutex_unlock(&e->mu);
            in_flight = 0;
        }
        r = take_output(e, in_flight, 1 << 30, pNals, iNalCount, out, NULL);
        e->st.output_ms += now_ms() - t0;
        const int ru = finish_upload(e);
        return r ? r : ru ? ru : e->sched_err;
    }
    /* flush: then every picture in flight is collected */
    const double t0 = now_ms();
    const int all = lane_flush_begin(e, 1);
    if (e->sched_err) return e->sched_err;
    r = take_output(e, all ? 0 : e->ring - 12, 1 << 30, pNals, iNalCount, out, NULL);
    e->st.output_ms += now_ms() - t0;
    return r;
}


/* extension: dump the encoder's reconstruction as I420, every picture at its display position (the reference CLI's -o).  Call right after
 * QY265EncoderOpen, before the first picture.  Costs one more D2H of W*H*3/2 bytes per picture: a checking aid, not part of the normal path. */
static int lane_recon_on(Enc *e)                                       /* the reconstruction of every picture comes back to the host (pinned, per job) */
{
    if (e->recon_on) return QY_OK;
    if (e->in_disp != 0) return QY_NOTSUPPORTED;
    e->key_overlap = 0;                                                /* the dump shares one device buffer: key pictures stay on the main stream */
    const size_t fsz = (size_t)e->W * e->H * 3 / 2;
    int r = ks265_dev_malloc(main_ctx(e), (void **)&e->dev_recon, fsz);
    for (int i = 0; i < e->ring && !r; ++i) r = ks265_host_malloc(main_ctx(e), (void **)&e->jobs[i].recon, fsz);
    if (r) return hip_rc(r);
    e->recon_on = 1;
    return QY_OK;
}
static int lane_set_recon_file(Enc *e, const char *path)
{
    if (!e || !path) return QY_POINTER;
    if (e->in_disp != 0 || e->recon_fd >= 0) return QY_NOTSUPPORTED;
    const int r = lane_recon_on(e);
    if (r) return r;
    e->recon_fd = open(path, O_WRONLY | O_CREAT | O_TRUNC, 0644);
    return e->recon_fd >= 0 ? QY_OK : QY_FAIL;
}

/* ------------------------------------------------------------------ GOP lanes
 * One lane (Enc) keeps one picture pipeline busy: a P picture needs its predecessor, so a single closed GOP fills about half of the MI355X (one stream
 * of the hot path runs at half the rate of three, bench.py).  Closed GOPs are independent - the shards of SURVEY.md 8(e) - so the encoder codes several of
 * them AT ONCE on one GPU: the handle owns L lanes, every lane a complete pipeline (streams, workspace, DPB, scheduler / dispatcher / writer threads);
 * GOP k of the input goes to lane k mod L, each GOP's first picture marked as a key picture in band; output is handed out in GOP order (all of GOP k,
 * then GOP k + 1 from the next lane), so the stream is byte for byte the one a single lane writes (tests/test_gpu_enc_api.py).  The reference's
 * enFrameParallel (frames of one stream coded concurrently on CPU threads) is the switch: lanes run with enFrameParallel != 0, fixed QP (-rc 0) and a key
 * period of at least 32 pictures (the rate controllers carry state across GOPs).  Every GOP structure works: the scheduler closes a GOP in front of a key picture
 * (the mini-GOP there is shortened to end in a P picture), so nothing references across lanes.  Cost: output lags the input by up to L GOPs, and L pipelines' worth of buffers.
 * Round 5: TWO lanes by default for the pyramid GOPs on one GPU (top_lanes_wanted: 631 -> 700 pictures/s at 2160p, GPU-bound at both), one otherwise.  IPPP, measured at 2160p
 * on the round-2 box: two lanes reach 1.05x of one (1123 vs 1068 frames/s; round 5: 890 against 970) -
 * with twice the pictures in flight the slice writers, not the GPU, set the pace (their time per picture grows from 19 to 59 ms of thread time as the
 * threads spread over the host), DESIGN.md section 6. */
#define MAX_LANES 16
#define MAX_CHUNKS 64
/* stash: pictures of a GOP that is not yet at the head of the output order are taken out of their lane as they finish (their NAL units copied here), so that the
 * lane's ring of pictures in flight never fills up with finished work waiting for an earlier GOP of another lane */
typedef struct Chunk {
    int lane, closed; long count, delivered, base; int disp0; /* the lane's own display index of the GOP's first picture */
    long stashed; QY265Nal *snal; size_t *soff; int sn, sn_cap; uint8_t *sbuf; size_t scap, spos; QY265Picture sout;
    ReconList srec;                                                  /* `devrecon`: the stashed pictures' reconstructions (their slots stay with them), in the order of snal */
} Chunk;
typedef struct Top {
    int nlanes; Enc *lane[MAX_LANES];
    int iper, key_request, cur_lane;
    long n_in, chunk_left;
    Chunk ch[MAX_CHUNKS]; int ch_head, ch_n;
    CopyPool *pool;
    QY265Nal *onals; size_t *ooff; int on, on_cap;                   /* output of the current call: NAL payloads copied out of the lanes */
    uint8_t *obuf; size_t ocap, opos;
    double output_ms;
    TopWake wake;
    ReconList handed;                                                /* `devrecon`: the reconstructions the last call handed out, in the order of its NAL units (ks265_recon.h) */
    ks265_roi roi; int roi_set;                                      /* `roi`: the map of the next picture handed in (ks265_enc_set_next_roi) */
    /* overlays (ks265_enc_set_overlay): the slots - d: as the device library takes it (a host overlay: pointing into `own`, its copy in device memory on lane 0's GPU, which
     * all lanes share read-only), stream: the caller's, for a device overlay - and the set built from them for the picture being handed in */
    struct OvSlot { int on, dev, forced_only; ks265_overlay_desc d; void *stream; void *own; } ov[KS265_OV_SLOTS];
    int ov_n, ov_warned; OvSet ovs;
    int tm_warned;                                        /* ks265_enc_enable_tonemap has logged that the device library lacks the entries */
} Top;

/* `devrecon`: what take_output just moved out of lane e's ring (Enc::taken) joins `dst` - the handle's list: the slots are handed out; a chunk's stash: they go on travelling.
 * c: the GOP the pictures belong to (lanes report their own display index), NULL with one lane */
static int recon_taken(Top *t, Enc *e, const Chunk *c, ReconList *dst)
{
    int r = QY_OK;
    for (int i = 0; i < e->taken.n; ++i) {
        ReconRef ref = e->taken.v[i];
        if (c) ref.poc = (int)(c->base + (ref.poc - c->disp0));
        if (dst == &t->handed) { pthread_mutex_lock(&e->mu); if (recon_pool_hand_out(&e->rpool, ref.slot)) r = QY_FAIL; pthread_mutex_unlock(&e->mu); }
        if (recon_list_push(dst, &ref)) r = QY_OUTOFMEMORY;
    }
    recon_list_clear(&e->taken);
    return r;
}
/* a stashed GOP goes out: its reconstructions are handed out behind what the call has handed out so far */
static int recon_unstash(Top *t, Chunk *c)
{
    Enc *e = t->lane[c->lane];
    int r = QY_OK;
    pthread_mutex_lock(&e->mu);
    for (int i = 0; i < c->srec.n; ++i) if (recon_pool_hand_out(&e->rpool, c->srec.v[i].slot)) r = QY_FAIL;
    pthread_mutex_unlock(&e->mu);
    if (recon_list_move(&t->handed, &c->srec)) r = QY_OUTOFMEMORY;
    return r;
}
/* the start of every call on the handle (and its close): every slot the previous call handed out goes back to its lane's pool, fetched or not */
static void recon_release(Top *t)
{
    if (!t->handed.n) return;
    for (int l = 0; l < t->nlanes; ++l) {
        Enc *e = t->lane[l];
        int any = 0;
        pthread_mutex_lock(&e->mu);
        for (int i = 0; i < t->handed.n; ++i) if (t->handed.v[i].lane == l) { (void)recon_pool_release(&e->rpool, t->handed.v[i].slot); any = 1; }
        if (any) pthread_cond_broadcast(&e->cv_done);                  /* the scheduler thread may be waiting for a slot (wait_recon_slot) */
        pthread_mutex_unlock(&e->mu);
    }
    recon_list_clear(&t->handed);
}

/* is there room for the picture whose first plane is `data`?  A slot in the caller's hands (4: ks265_enc_acquire_input) counts only if THIS picture is the one that was
 * produced into it - a caller may acquire a buffer and then hand in its own, or the picture may be routed to another lane */
static int lane_has_slot(Enc *e, const uint8_t *data)
{
    int ok = 0;
    pthread_mutex_lock(&e->mu);
    for (int i = 0; i < e->nin && !ok; ++i) ok = e->in[i].used == IN_FREE || (e->in[i].used == IN_ACQUIRED && e->in[i].i420 == data);
    pthread_mutex_unlock(&e->mu);
    return ok;
}

static int nal_append(QY265Nal **dn, size_t **doff, int *dcnt, int *dcap, uint8_t **dbuf, size_t *bcap, size_t *bpos, const QY265Nal *nals, int n)
{
    for (int i = 0; i < n; ++i) {
        if (*dcnt == *dcap) {
            const int nc = *dcap ? 2 * *dcap : 1024;
            QY265Nal *a = (QY265Nal *)realloc(*dn, (size_t)nc * sizeof *a);
            if (a) *dn = a;
            size_t *b = a ? (size_t *)realloc(*doff, (size_t)nc * sizeof *b) : NULL;
            if (!a || !b) return QY_OUTOFMEMORY;
            *doff = b; *dcap = nc;
        }
        const size_t need = (size_t)nals[i].iSize;
        if (*bpos + need > *bcap) {
            const size_t nc = (*bpos + need) * 2 + 65536;
            uint8_t *nb = (uint8_t *)realloc(*dbuf, nc);
            if (!nb) return QY_OUTOFMEMORY;
            *dbuf = nb; *bcap = nc;
        }
        memcpy(*dbuf + *bpos, nals[i].pPayload, need);
        (*dn)[*dcnt] = nals[i]; (*doff)[*dcnt] = *bpos;
        ++*dcnt; *bpos += need;
    }
    return QY_OK;
}
static int top_append(Top *t, const QY265Nal *nals, int n) { return nal_append(&t->onals, &t->ooff, &t->on, &t->on_cap, &t->obuf, &t->ocap, &t->opos, nals, n); }

/* move finished pictures to the call's output, GOP after GOP; block = wait until at least one picture has come */
static int top_collect_pass(Top *t, QY265Picture *out, long *progress, long *pending)
{
    while (t->ch_n) {
        Chunk *c = &t->ch[t->ch_head];
        if (c->sn) {                                                    /* what was taken out of the lane while earlier GOPs were still going out */
            for (int i = 0; i < c->sn; ++i) c->snal[i].pPayload = c->sbuf + c->soff[i];
            const int ra = top_append(t, c->snal, c->sn);
            if (ra) return ra;
            const int rr = recon_unstash(t, c);
            if (rr) return rr;
            c->delivered += c->stashed; *progress += c->stashed; c->stashed = 0; c->sn = 0; c->spos = 0;
            if (out) { out->iSliceType = c->sout.iSliceType; out->pts = c->sout.pts; out->dts = c->sout.dts; out->poc = (int)(c->base + (c->sout.poc - c->disp0)); }
        }
        if (c->delivered == c->count) {
            if (!c->closed) break;                                      /* the GOP still receives input */
            free(c->snal); free(c->soff); free(c->sbuf); c->snal = NULL; c->soff = NULL; c->sbuf = NULL; c->sn_cap = 0; c->scap = 0;
            recon_list_free(&c->srec);
            t->ch_head = (t->ch_head + 1) % MAX_CHUNKS; --t->ch_n;
            continue;
        }
        QY265Nal *nals; int n = 0, pics = 0;
        const int r = take_output(t->lane[c->lane], MAX_JOBS + 1, (int)(c->count - c->delivered), &nals, &n, out, &pics);
        /* (a picture that failed on the device has left the lane's ring like any other - without a payload: it is on the books before the error goes up, or this GOP
         *  would wait for it for ever) */
        const int ra = pics ? top_append(t, nals, n) : QY_OK;
        const int rr = recon_taken(t, t->lane[c->lane], c, &t->handed);
        c->delivered += pics; *progress += pics;
        if (r) return r;
        if (ra) return ra;
        if (rr) return rr;
        if (!pics) break;
        if (out) out->poc = (int)(c->base + (out->poc - c->disp0));    /* the lane reports its own display index */
    }
    /* the GOPs behind the head: whatever their lanes have finished goes into the stash (a lane hands its pictures out in its own order: only its oldest unfinished
     * GOP can be taken from) */
    unsigned busy = 0;                                                  /* lanes whose oldest unfinished GOP has been seen */
    for (int k = 0; k < t->ch_n; ++k) {
        Chunk *c = &t->ch[(t->ch_head + k) % MAX_CHUNKS];
        *pending += c->count - c->delivered - c->stashed;
        if (busy >> c->lane & 1u) continue;
        if (c->delivered + c->stashed == c->count && c->closed) continue;   /* all taken: the lane's next GOP is its oldest unfinished one */
        busy |= 1u << c->lane;
        if (k == 0) continue;                                           /* the head goes out directly (above) */
        for (;;) {
            const long left = c->count - c->delivered - c->stashed;
            if (left <= 0) break;
            QY265Nal *nals; int n = 0, pics = 0;
            const int r = take_output(t->lane[c->lane], MAX_JOBS + 1, (int)left, &nals, &n, &c->sout, &pics);
            const int ra = pics ? nal_append(&c->snal, &c->soff, &c->sn, &c->sn_cap, &c->sbuf, &c->scap, &c->spos, nals, n) : QY_OK;
            const int rr = recon_taken(t, t->lane[c->lane], c, &c->srec);
            c->stashed += pics; *progress += pics; *pending -= pics;
            if (r) return r;
            if (ra) return ra;
            if (rr) return rr;
            if (!pics) break;
        }
    }
    return QY_OK;
}

/* move finished pictures to the call's output, GOP after GOP (and, from the lanes behind, to their stash); block = do not come back before SOMETHING has moved
 * (a picture out, or into a stash: either frees a lane's buffers), unless nothing is on its way at all */
static int top_collect(Top *t, int block, QY265Picture *out)
{
    for (;;) {
        pthread_mutex_lock(&t->wake.mu);
        const unsigned long seen = t->wake.seq;
        pthread_mutex_unlock(&t->wake.mu);
        long progress = 0, pending = 0;
        const int r = top_collect_pass(t, out, &progress, &pending);
        if (r || !block || progress || !pending) return r;
        for (int i = 0; i < t->nlanes; ++i) {
            Enc *e = t->lane[i];
            pthread_mutex_lock(&e->mu);
            const int bad = e->quit ? QY_FAIL : e->sched_err;
            pthread_mutex_unlock(&e->mu);
            if (bad) return bad;
        }
        pthread_mutex_lock(&t->wake.mu);
        if (t->wake.seq == seen) {                                      /* a writer thread of any lane finishing a picture wakes this up; the time limit covers a failing lane */
            struct timespec ts; clock_gettime(CLOCK_REALTIME, &ts);
            ts.tv_nsec += 20 * 1000000L; if (ts.tv_nsec >= 1000000000L) { ts.tv_nsec -= 1000000000L; ++ts.tv_sec; }
            pthread_cond_timedwait(&t->wake.cv, &t->wake.mu, &ts);
        }
        pthread_mutex_unlock(&t->wake.mu);
    }
}

/* no more input for the newest GOP.  early: it ends before its period is over (a key-picture request) - with B pictures the lane's scheduler is still waiting
 * for the rest of a mini-GOP, so it is told where the GOP ends (short mini-GOP there, as in front of a key picture); a GOP of full length ends by itself */
static void top_close_chunk(Top *t, int early)
{
    Chunk *c = &t->ch[(t->ch_head + t->ch_n - 1) % MAX_CHUNKS];
    c->closed = 1;
    if (t->lane[c->lane]->la_on) (void)la_drain(t->lane[c->lane], 0);  /* the GOP's last pictures do not wait for the lane's next ones (an error is in sched_err) */
    if (early) {
        Enc *e = t->lane[c->lane];
        pthread_mutex_lock(&e->mu);
        e->gop_end = e->in_disp - 1;                                  /* the lane's own index of the GOP's last picture */
        pthread_cond_signal(&e->cv_sched);
        pthread_mutex_unlock(&e->mu);
    }
}

/* The GPUs of this handle: KS265_DEVICES = "0,2,5" (an explicit list) or KS265_GPUS = N (devices 0 .. N - 1; the CLI's -gpus N), else KS265_DEVICE / 0.
 * Closed GOPs are independent ("frames / GOPs shard naturally across the GPUs of one node", no data-path collective), so a GPU is simply another
 * GOP lane: lane i runs on device dev[i mod ndev], KS265_GOP_LANES lanes per GPU.  The stream is byte for byte the one-GPU stream. */
static int top_devices(int dev[MAX_LANES])
{
    int n = 0;
    const char *list = getenv("KS265_DEVICES"), *cnt = getenv("KS265_GPUS"), *one = getenv("KS265_DEVICE");
    if (list && *list) {
        const char *p = list;
        while (*p && n < MAX_LANES) {
            char *end; const long v = strtol(p, &end, 10);
            if (end == p) break;
            if (v >= 0 && v < 1024) dev[n++] = (int)v;
            p = *end == ',' ? end + 1 : end;
        }
    } else if (cnt && atoi(cnt) > 0) { for (int i = 0; i < atoi(cnt) && i < MAX_LANES; ++i) dev[n++] = i; }
    if (!n) dev[n++] = one ? atoi(one) : 0;
    return n;
}
static int top_lanes_wanted(const QY265EncConfig *cfg, int ndev)
{
    /* one lane per GPU unless asked (round 6): two closed GOPs side by side fill what the B pictures of a pyramid GOP leave of the device (2160p: 700 pictures/s
     * against 631), but a lane runs a whole GOP behind its input - twice the lag and twice the pinned input of one - and needs more than the runtime's four hardware queues
     * (GPU_MAX_HW_QUEUES=8, exported BEFORE the process first touches the GPU; with four: 561).  Both are the application's decisions: the CLI and bench.py take them
     * (KS265_GOP_LANES=2 + GPU_MAX_HW_QUEUES=8 for the pyramid GOPs under -rc 0 / 3), the library never changes the environment. */
    const char *env = getenv("KS265_GOP_LANES");
    int per = env ? atoi(env) : 1;
    if (per > 1) {
        const char *q = getenv("GPU_MAX_HW_QUEUES");
        if (!q || atoi(q) < 8) logf_(1, cfg->logLevel, "ks265enc: %d GOP lanes with %s hardware queues: export GPU_MAX_HW_QUEUES=8 before the process first uses the GPU (measured: two lanes on four queues are slower than one)\n", per, q ? q : "the runtime's default four");
    }
    if (per < 1) per = 1;
    int n = per * ndev;
    if (n > MAX_LANES) n = MAX_LANES;
    /* closed GOPs share no pixel; what a rate-control mode shares across GOPs decides whether they can be dealt to lanes:
     *   rc 0 (constant QP) and rc 3 (CRF = a constant ladder on crf): nothing - the lanes' stream is byte for byte the one-lane stream;
     *   rc 1 / 2 / 4 (bitrate targets): the controller's state.  With lanes every lane runs its OWN controller on the GOPs dealt to it, each picture carrying the same
     *   budget share (bitrate / frame rate, rc_account): the host-side bit-budget split of SURVEY.md 8(e) - a scalar per picture, no exchange between GPUs.  The
     *   stream is deterministic for a given lane count but not the one-lane stream (a lane's offset follows the GOPs it has seen), which the open logs;
     *   rc 5 / VBV are not implemented at all.  -md5 lines are in one display order: one lane. */
    if (!cfg->enFrameParallel || cfg->rc < 0 || cfg->rc > 4 || cfg->iIntraPeriod < 32 || g_cli.md5) n = 1;
    if (cfg->lookahead > 0) n = 1;                                   /* a scene cut restarts the key period: GOP boundaries are not known when the pictures are dealt to lanes */
    return n;
}

void *QY265EncoderOpen(QY265EncConfig *cfg, int *err)
{
    int dummy; if (!err) err = &dummy;
    *err = QY_OK;
    if (!cfg) { *err = QY_POINTER; return NULL; }
    Top *t = (Top *)calloc(1, sizeof *t);
    if (!t) { *err = QY_OUTOFMEMORY; return NULL; }
    int dev[MAX_LANES];
    const int ndev = top_devices(dev);
    t->nlanes = top_lanes_wanted(cfg, ndev);
    if (ndev > 1 && t->nlanes == 1) logf_(2, cfg->logLevel, "ks265enc: %d GPUs asked for, but GOP sharding needs enFrameParallel, -rc 0..4, no -lookahead / -md5 and a key period >= 32: one GPU\n", ndev);
    if (t->nlanes > 1 && (cfg->rc == 1 || cfg->rc == 2 || cfg->rc == 4))
        logf_(1, cfg->logLevel, "ks265enc: -rc %d over %d GOP lanes: every lane runs its own controller with the same per-picture bit budget (deterministic, not the one-lane stream)\n", cfg->rc, t->nlanes);
    t->iper = cfg->iIntraPeriod; t->cur_lane = -1;
    QY265EncConfig lc = *cfg;
    if (t->nlanes > 1) {                                                /* the writer threads are shared out: every lane sees 1 / L of the pictures */
        long ncpu = sysconf(_SC_NPROCESSORS_ONLN);
        /* the host's threads are the budget: every lane also runs a scheduler, a dispatcher (polling) and shares the copy helpers - three service threads apiece;
         * what is left is dealt to the lanes as slice writers, at most 32 each (one GPU's pictures keep about that many busy) */
        const int th = cfg->threads > 0 ? cfg->threads : (int)(ncpu > 0 ? ncpu : 4) - 3 * t->nlanes;    /* an explicit -threads is the total */
        lc.threads = th / t->nlanes;
        if (lc.threads > 32) lc.threads = 32;
        if (lc.threads < 2) lc.threads = 2;
    }
    int spread = 0;
    for (int i = 1; i < t->nlanes; ++i) if (dev[i % ndev] != dev[0]) spread = 1;
    for (int i = 0; i < t->nlanes; ++i) {
        if (i) lc.logLevel = cfg->logLevel > 2 ? cfg->logLevel : 3;     /* one start-up line */
        t->lane[i] = lane_open(&lc, dev[i % ndev], t->nlanes > 1 ? 1 + spread : 0, err);   /* (2: lanes on several GPUs - lane_resolve's `devrecon`) */
        if (!t->lane[i]) {
            if (i == 0) { free(t); return NULL; }
            t->nlanes = i;                                              /* e.g. out of memory for another pipeline: go on with the lanes there are */
            *err = QY_OK;
            break;
        }
    }
    if ((size_t)cfg->picWidth * cfg->picHeight >= ((size_t)1 << 20)) t->pool = copy_pool_create();
    pthread_mutex_init(&t->wake.mu, NULL); pthread_cond_init(&t->wake.cv, NULL);
    for (int i = 0; i < t->nlanes; ++i) { t->lane[i]->lane_idx = i; t->lane[i]->pool = t->pool; t->lane[i]->multi = t->nlanes > 1; t->lane[i]->wake = t->nlanes > 1 ? &t->wake : NULL; }
    if (t->nlanes > 1) logf_(0, cfg->logLevel, "ks265enc: %d GOP lanes on %d GPU(s) (closed GOPs of %d pictures coded concurrently, output in GOP order)\n", t->nlanes, ndev < t->nlanes ? ndev : t->nlanes, t->iper);
    return t;
}

/* a slot is emptied: what pictures in flight still read of a host overlay's copy is waited for (every lane's upload stream), then the copy goes */
static void overlay_drop(Top *t, int k)
{
    struct OvSlot *o = &t->ov[k];
    if (o->own) {
        for (int i = 0; i < t->nlanes; ++i) if (t->lane[i]->ctx_up) (void)ks265_synchronize(t->lane[i]->ctx_up);
        ks265_dev_free(main_ctx(t->lane[0]), o->own);
    }
    if (o->on) --t->ov_n;
    memset(o, 0, sizeof *o);
}

void QY265EncoderClose(void *h)
{
    Top *t = (Top *)h;
    if (!t) return;
    if (t->nlanes > 1) {                                                /* one summary line over all lanes */
        Enc *e0 = t->lane[0];
        ks265_enc_stats st; memset(&st, 0, sizeof st);
        for (int i = 0; i < t->nlanes; ++i) { const ks265_enc_stats *s = &t->lane[i]->st; st.frames += s->frames; st.bytes += s->bytes; for (int k = 0; k < 3; ++k) st.sse[k] += s->sse[k]; }
        long long hi[3] = {0, 0, 0}, lo[3] = {0, 0, 0};
        for (int i = 0; i < t->nlanes; ++i) for (int k = 0; k < 3; ++k) { hi[k] += t->lane[i]->q_hi[k]; lo[k] += t->lane[i]->q_lo[k]; }
        run_summary(e0, st.frames, st.bytes, st.sse, hi, lo);
    }
    recon_release(t);
    for (int k = 0; k < KS265_OV_SLOTS; ++k) overlay_drop(t, k);         /* (the host overlays' copies, behind the pictures that read them) */
    for (int i = 0; i < t->nlanes; ++i) lane_close(t->lane[i], t->nlanes == 1);
    recon_list_free(&t->handed);
    pthread_mutex_destroy(&t->wake.mu); pthread_cond_destroy(&t->wake.cv);
    copy_pool_destroy(t->pool);
    for (int i = 0; i < MAX_CHUNKS; ++i) { free(t->ch[i].snal); free(t->ch[i].soff); free(t->ch[i].sbuf); recon_list_free(&t->ch[i].srec); }
    free(t->onals); free(t->ooff); free(t->obuf);
    free(t);
}

void QY265EncoderReconfig(void *h, QY265EncConfig *cfg)
{
    Top *t = (Top *)h;
    if (!t || !cfg) return;
    for (int i = 0; i < t->nlanes; ++i) lane_reconfig(t->lane[i], cfg);
    if (t->nlanes > 1 && cfg->iIntraPeriod >= 1) t->iper = cfg->iIntraPeriod;
}
int QY265EncoderEncodeHeaders(void *h, QY265Nal **pNals, int *n)
{
    Top *t = (Top *)h;
    if (!t || !pNals || !n) return QY_POINTER;
    return lane_headers(t->lane[0], pNals, n);
}
void QY265EncoderKeyFrameRequest(void *h)
{
    Top *t = (Top *)h;
    if (!t) return;
    if (t->nlanes == 1) t->lane[0]->force_key = 1; else t->key_request = 1;   /* lanes: the next picture opens a new GOP on the next lane */
}
int QY265EncoderDelayedFrames(void *h)
{
    Top *t = (Top *)h;
    if (!t) return 0;
    int n = 0;
    for (int i = 0; i < t->nlanes; ++i) n += lane_delayed(t->lane[i]);
    for (int k = 0; k < t->ch_n; ++k) n += (int)t->ch[(t->ch_head + k) % MAX_CHUNKS].stashed;   /* taken out of their lane, waiting for an earlier GOP to go out */
    return n;
}

/* the lane the NEXT picture goes to: a new GOP starts on the next lane (top_encode, ks265_enc_acquire_input, ks265_enc_encode_device_frame_scaled) */
static int top_next_lane(const Top *t) { return t->nlanes == 1 ? 0 : (t->chunk_left <= 0 || t->key_request) ? (t->cur_lane + 1) % t->nlanes : t->cur_lane; }

/* the overlays of the picture being handed in: the slots that are set, ascending, a forced-only one if the call forced the logo; p->ovs stays NULL if that leaves none */
static void top_overlay_set(Top *t, PicIn *p)
{
    OvSet *s = &t->ovs;
    s->n = s->nst = 0;
    for (int k = 0; k < KS265_OV_SLOTS; ++k) {
        const struct OvSlot *o = &t->ov[k];
        if (!o->on || (o->forced_only && !p->force_logo)) continue;
        s->d[s->n++] = o->d;
        int seen = !o->dev;
        for (int j = 0; j < s->nst && !seen; ++j) seen = s->stream[j] == o->stream;
        if (!seen) s->stream[s->nst++] = o->stream;
    }
    if (s->n) p->ovs = s;
}

/* one call of the API: a picture (p) or, NULL, the flush */
static int top_encode(Top *t, QY265Nal **pNals, int *iNalCount, PicIn *p, QY265Picture *out)
{
    recon_release(t);                                                 /* `devrecon`: the previous call's reconstructions are the pool's again */
    if (p) { p->roi = t->roi_set ? &t->roi : NULL; t->roi_set = 0; }    /* `roi`: the pending map goes with this picture - whatever becomes of the call, nothing stays pending (a flush: it stays) */
    if (p && t->ov_n) top_overlay_set(t, p);                            /* overlays: the set in force goes with this picture, into whichever lane takes it */
    if (t->nlanes == 1) {
        const int r1 = lane_encode_frame(t->lane[0], pNals, iNalCount, p, out);
        const int rr = t->lane[0]->pool_on ? recon_taken(t, t->lane[0], NULL, &t->handed) : QY_OK;
        return r1 ? r1 : rr;
    }
    *pNals = NULL; *iNalCount = 0;
    t->on = 0; t->opos = 0;
    int r = QY_OK;
    if (p) {
        int first = 0;
        const int next = top_next_lane(t);
        if (t->chunk_left <= 0 || t->key_request) {                     /* a new GOP: the next lane */
            if (t->ch_n) top_close_chunk(t, t->chunk_left > 0);
            while (t->ch_n == MAX_CHUNKS && !r) r = top_collect(t, 1, out);
            if (r) return r;
            t->cur_lane = next;
            Chunk *c = &t->ch[(t->ch_head + t->ch_n) % MAX_CHUNKS];
            memset(c, 0, sizeof *c);
            c->lane = t->cur_lane; c->base = t->n_in; c->disp0 = t->lane[t->cur_lane]->in_disp;
            ++t->ch_n;
            t->chunk_left = t->iper > 0 ? t->iper : (1L << 40);
            t->key_request = 0; first = 1;
        }
        Enc *e = t->lane[t->cur_lane];
        const double t0 = now_ms();
        while (!lane_has_slot(e, p->yuv ? p->yuv->pData[0] : NULL)) {                                     /* this lane is as far ahead as its buffers allow: finish older GOPs first */
            r = top_collect(t, 1, out);
            if (r) return r;
        }
        t->output_ms += now_ms() - t0;
        r = lane_put(e, p, first);
        if (r) return r;
        ++t->ch[(t->ch_head + t->ch_n - 1) % MAX_CHUNKS].count; ++t->n_in; --t->chunk_left;
        const double t1 = now_ms();
        r = top_collect(t, 0, out);
        t->output_ms += now_ms() - t1;
        const int ru = finish_upload(e); if (!r) r = ru;
        if (!r) for (int i = 0; i < t->nlanes && !r; ++i) r = t->lane[i]->sched_err;
    } else {
        const double t0 = now_ms();
        if (t->ch_n) top_close_chunk(t, 0);                              /* the lanes are flushed below */
        t->chunk_left = 0;
        for (int i = 0; i < t->nlanes; ++i) {
            if (lane_delayed(t->lane[i])) lane_flush_begin(t->lane[i], 0);
            if (t->lane[i]->sched_err) return t->lane[i]->sched_err;
        }
        r = top_collect(t, 1, out);
        t->output_ms += now_ms() - t0;
    }
    for (int i = 0; i < t->on; ++i) t->onals[i].pPayload = t->obuf + t->ooff[i];
    *pNals = t->onals; *iNalCount = t->on;
    return r;
}

int QY265EncoderEncodeFrame(void *h, QY265Nal **pNals, int *iNalCount, QY265Picture *in, QY265Picture *out, int bForceLogo)
{
    Top *t = (Top *)h;
    if (!t || !pNals || !iNalCount) return QY_POINTER;
    PicIn p = {.how = PIC_HOST, .yuv = in ? in->yuv : NULL, .pts = in ? in->pts : 0, .force_logo = bForceLogo != 0};   /* (bForceLogo: KS265_OV_FORCED_ONLY overlays alone look at it) */
    return top_encode(t, pNals, iNalCount, in ? &p : NULL, out);
}

int ks265_enc_get_stats(void *h, ks265_enc_stats *out)
{
    Top *t = (Top *)h;
    if (!t || !out) return QY_POINTER;
    *out = t->lane[0]->st;
    for (int i = 1; i < t->nlanes; ++i) {                               /* sums over the lanes (per-picture averages divide by frames as before) */
        const ks265_enc_stats *s = &t->lane[i]->st;
        out->frames += s->frames; out->bytes += s->bytes;
        for (int k = 0; k < 3; ++k) out->sse[k] += s->sse[k];
        out->gpu_ms += s->gpu_ms; out->host_write_ms += s->host_write_ms; out->in_copy_ms += s->in_copy_ms; out->submit_ms += s->submit_ms;
        out->lat_gpu_ms += s->lat_gpu_ms; out->lat_queue_ms += s->lat_queue_ms; out->key_wall_ms += s->key_wall_ms; out->key_cpu_ms += s->key_cpu_ms; out->keys += s->keys;
        out->submit_wait_ms += s->submit_wait_ms; out->occ_samples += s->occ_samples; out->occ_ring += s->occ_ring; out->occ_gpu += s->occ_gpu; out->occ_ready += s->occ_ready;
    }
    if (t->nlanes > 1) out->output_ms = t->output_ms;
    return QY_OK;
}

int ks265_enc_get_quality(void *h, ks265_enc_quality *out)
{
    Top *t = (Top *)h;
    if (!t || !out) return QY_POINTER;
    memset(out, 0, sizeof *out);
    const Enc *e0 = t->lane[0], *last = NULL;
    const double nw[3] = {(double)(e0->W / 8) * (e0->H / 8), (double)(e0->W / 16) * (e0->H / 16), (double)(e0->W / 16) * (e0->H / 16)};
    long long hi[3] = {0, 0, 0}, lo[3] = {0, 0, 0};
    out->last_poc = -1;
    for (int i = 0; i < t->nlanes; ++i) {
        Enc *e = t->lane[i];
        pthread_mutex_lock(&e->mu);
        out->frames += e->st.frames;
        for (int k = 0; k < 3; ++k) { out->sse[k] += e->st.sse[k]; hi[k] += e->q_hi[k]; lo[k] += e->q_lo[k]; }
        if (e->st.frames && (!last || e->q_seq > last->q_seq)) {
            last = e; out->last_poc = e->q_last_poc;
            for (int k = 0; k < 3; ++k) { out->last_sse[k] = e->q_last_sse[k]; out->last_ssim[k] = e->q_last_ssim[k]; }
        }
        pthread_mutex_unlock(&e->mu);
    }
    out->have_sse = e0->cfg.calcPsnr != 0; out->have_ssim = e0->ssim_on;
    for (int k = 0; k < 3; ++k) out->ssim[k] = e0->ssim_on && nw[k] > 0 ? ((double)hi[k] + (double)lo[k] / 1073741824.0) / nw[k] : 0.0;
    return QY_OK;
}

int ks265_enc_lanes(void *h) { const Top *t = (const Top *)h; return t ? t->nlanes : 0; }

int ks265_enc_acquire_input(void *h, QY265YUV *yuv)
{
    Top *t = (Top *)h;
    if (!t || !yuv) return QY_POINTER;
    return lane_acquire(t->lane[top_next_lane(t)], yuv);
}

/* every input slot of the lane gets a device twin (and the event behind its filling) if it has none yet, and the lane a stream for filling them: the lookahead's when there is one
 * (its analysis reads the twin right after), else the pixel path's - no stream more (a stream more is a hardware queue shared with somebody, lane_open) */
static int lane_make_twins(Enc *e)
{
    if (!e->ctx_up) { e->ctx_up = e->ctx_la ? e->ctx_la : main_ctx(e); reg_handle(main_ctx(e), 1); }     /* (lane_close lets go of the registrations of every lane with a ctx_up) */
    const size_t fsz = (size_t)e->W * e->H * 3 / 2;
    int r = KS265_OK;
    for (int i = 0; i < e->nin && !r; ++i) {
        if (!e->in[i].dev) r = ks265_dev_malloc(main_ctx(e), (void **)&e->in[i].dev, fsz);
        if (!r && !e->in[i].ev_up) r = ks265_event_create(e->ctx_up, &e->in[i].ev_up);
    }
    return hip_rc(r);
}
static int lane_enable_device_input(Enc *e)
{
    if (e->dev_in_on) return QY_OK;
    const int r = lane_make_twins(e);
    if (r) return r;
    e->dev_in_on = 1;
    return QY_OK;
}
/* overlays need the twins too.  A lane that has them all is fine as it is; one that has none may get them only while no picture is in flight: the scheduler thread reads a
 * slot's twin pointer when it takes the picture, and a picture handed in without a twin has its bytes in pinned memory alone */
static int lane_twins_missing(const Enc *e) { for (int i = 0; i < e->nin; ++i) if (!e->in[i].dev || !e->in[i].ev_up) return 1; return 0; }
static int lane_idle(Enc *e)
{
    pthread_mutex_lock(&e->mu);
    int idle = 1;
    for (int i = 0; i < e->nin; ++i) if (e->in[i].used != IN_FREE && e->in[i].used != IN_ACQUIRED) idle = 0;
    pthread_mutex_unlock(&e->mu);
    return idle;
}

int ks265_enc_enable_device_input(void *h)
{
    Top *t = (Top *)h;
    if (!t) return QY_POINTER;
    if (!ks265_input_validate || !ks265_input_convert || !ks265_wait_external || !ks265_external_wait_event) return QY_NOTSUPPORTED;   /* a device library without the conversion */
    for (int i = 0; i < t->nlanes; ++i) {
        const Enc *e = t->lane[i];
        if (e->in_disp || e->dev_id != t->lane[0]->dev_id || e->use_graph) return QY_NOTSUPPORTED;   /* after the first picture; lanes on several GPUs; the graph experiment (captures on the pixel path's stream) */
    }
    for (int i = 0; i < t->nlanes; ++i) { const int r = lane_enable_device_input(t->lane[i]); if (r) return r; }
    return QY_OK;
}

/* the lane's plan for (source size, filter) into *out: the cached one, or a new one in the place of the least recently used - created here, on the caller's thread; the one that
 * goes may still be read by a picture in flight on ctx_up, which is waited for first.  More than SCALE_PLANS sizes in turn pay that wait and the tables with every picture */
static int lane_scale_plan(Enc *e, int sw, int sh, int filter, const struct ScalePlan **out)
{
    int at = -1;
    for (int i = 0; i < SCALE_PLANS; ++i)
        if (e->sc_plan[i].plan && e->sc_plan[i].sw == sw && e->sc_plan[i].sh == sh && e->sc_plan[i].filter == filter) { e->sc_plan[i].used = ++e->sc_tick; *out = &e->sc_plan[i]; return KS265_OK; }
    for (int i = 0; i < SCALE_PLANS && at < 0; ++i) if (!e->sc_plan[i].plan) at = i;
    for (int i = 0; i < SCALE_PLANS && (at < 0 || e->sc_plan[at].plan); ++i) if (at < 0 || e->sc_plan[i].used < e->sc_plan[at].used) at = i;
    ks265_scale_plan *np = NULL;
    const int r = ks265_scale_plan_create(main_ctx(e), sw, sh, e->W, e->H, filter, &np);
    if (r) return r;
    if (e->sc_plan[at].plan) { (void)ks265_synchronize(e->ctx_up); (void)ks265_scale_plan_destroy(main_ctx(e), e->sc_plan[at].plan); }
    e->sc_plan[at].plan = np; e->sc_plan[at].sw = sw; e->sc_plan[at].sh = sh; e->sc_plan[at].filter = filter; e->sc_plan[at].used = ++e->sc_tick;
    *out = &e->sc_plan[at];
    return KS265_OK;
}

int ks265_enc_enable_device_scale(void *h, int max_src_width, int max_src_height)
{
    Top *t = (Top *)h;
    if (!t) return QY_POINTER;
    Enc *e0 = t->lane[0];
    if (!e0->dev_in_on) return QY_NOTSUPPORTED;
    for (int i = 0; i < t->nlanes; ++i) if (t->lane[i]->in_disp) return QY_NOTSUPPORTED;   /* after the first picture */
    if (!ks265_scale_plan_create || !ks265_scale_plan_destroy || !ks265_input_scale) {
        logf_(2, e0->log_level, "ks265enc: input scaling is unavailable: the device library has no ks265_input_scale\n");
        return QY_NOTSUPPORTED;
    }
    if (max_src_width <= 0 || max_src_height <= 0 || (max_src_width & 7) || (max_src_height & 1) || max_src_width > KS_SCALE_MAX_DIM || max_src_height > KS_SCALE_MAX_DIM
        || max_src_width > KS_SCALE_MAX_RATIO * e0->W || max_src_height > KS_SCALE_MAX_RATIO * e0->H || (e0->W & 7) || (e0->H & 7) || e0->ragged) return QY_NOTSUPPORTED;
    if (e0->sc_on) return e0->sc_max_w == max_src_width && e0->sc_max_h == max_src_height ? QY_OK : QY_NOTSUPPORTED;
    for (int i = 0; i < t->nlanes; ++i) {
        Enc *e = t->lane[i];
        e->sc_max_w = max_src_width; e->sc_max_h = max_src_height;
        const int r = open_scale(e);
        if (r) { for (int k = 0; k < i; ++k) { close_scale(t->lane[k]); t->lane[k]->sc_on = 0; } return hip_rc(r); }   /* lane i itself got nothing */
        e->sc_on = 1;
    }
    return QY_OK;
}

/* a device picture resolved into *p: the operation that makes the slot's twin of it - scaled (from sw x sh, a size that is not the lane's), padded on a ragged handle, else converted - its view of the picture,
 * validated, and for scaling the plan.  All of it before anything is enqueued or counted: a refused picture leaves the handle as it was (a pending ROI map too) */
static int resolve_device(Top *t, const ks265_dev_picture *pic, int scaled, int sw, int sh, int filter, PicIn *p)
{
    Enc *e0 = t->lane[0];
    *p = (PicIn){.how = scaled ? PIC_SCALE : e0->ragged ? PIC_PAD : PIC_CONVERT, .dp = pic, .pts = pic->pts};
    if ((p->how == PIC_SCALE ? !e0->sc_on : !e0->dev_in_on || !ks265_input_validate) || pic->device != e0->dev_id) return QY_NOTSUPPORTED;
    if (p->how == PIC_SCALE && (!ks265_scale_size_ok(sw, sh, e0->W, e0->H) || sw > e0->sc_max_w || sh > e0->sc_max_h || (filter != KS_SCALE_TRIANGLE && filter != KS_SCALE_CATMULL_ROM))) return QY_NOTSUPPORTED;
    const double t0 = now_ms();
    dev_desc(e0, pic, &p->d);
    if (p->how == PIC_SCALE) { p->d.width = sw; p->d.height = sh; }
    if (p->how == PIC_PAD && p->d.format != KS265_IN_I420 && p->d.format != KS265_IN_NV12) return QY_NOTSUPPORTED;   /* a ragged handle pads 8-bit I420 and NV12 only (ks265_enc.h) */
    /* a tone-mapping handle: YUV of more than 8 bits is mapped when it is 4:2:0, planar or semi-planar, of 10 to 16 bits - and refused otherwise, never passed through unmapped */
    if (e0->tm_on && (p->d.format & ~0x3FF) == 0x1000 && (p->d.format & 31) > 8) {
        if (!ks265_tm_format_ok(p->d.format >> 8 & 3, p->d.format >> 6 & 3, p->d.format & 31)) return QY_NOTSUPPORTED;
        p->tm = 1;
    }
    int rv = p->tm ? ks265_input_tonemap_validate(main_ctx(e0), e0->tm_plan, &p->d) : p->how == PIC_PAD ? ks265_input_pad_validate(main_ctx(e0), &p->d, e0->W, e0->H) : ks265_input_validate(main_ctx(e0), &p->d);
    if (!rv && p->how == PIC_SCALE) rv = lane_scale_plan(t->lane[top_next_lane(t)], sw, sh, filter, &p->sc);
    e0->st.in_copy_ms += now_ms() - t0;
    return hip_rc(rv);
}
static int encode_device(void *h, QY265Nal **pNals, int *iNalCount, const ks265_dev_picture *pic, int scaled, int sw, int sh, int filter, QY265Picture *out)
{
    Top *t = (Top *)h;
    if (!t || !pNals || !iNalCount || !pic) return QY_POINTER;
    *iNalCount = 0;
    if (scaled && t->lane[0]->ragged) return QY_NOTSUPPORTED;               /* the scaler writes coded sizes only (ks265_enc.h) */
    if (sw == t->lane[0]->W && sh == t->lane[0]->H) scaled = 0;           /* a source of the encoder's own size IS ks265_enc_encode_device_frame */
    PicIn p;
    const int r = resolve_device(t, pic, scaled, sw, sh, filter, &p);
    return r ? r : top_encode(t, pNals, iNalCount, &p, out);
}
int ks265_enc_encode_device_frame(void *h, QY265Nal **pNals, int *iNalCount, const ks265_dev_picture *pic, QY265Picture *out) { return encode_device(h, pNals, iNalCount, pic, 0, 0, 0, 0, out); }
int ks265_enc_encode_device_frame_scaled(void *h, QY265Nal **pNals, int *iNalCount, const ks265_dev_picture *pic, int src_width, int src_height, int filter, QY265Picture *out) { return encode_device(h, pNals, iNalCount, pic, 1, src_width, src_height, filter, out); }

int ks265_enc_enable_tonemap(void *h, const ks265_tonemap *tm)
{
    Top *t = (Top *)h;
    if (!t || !tm) return QY_POINTER;
    Enc *e0 = t->lane[0];
    if (!ks265_tonemap_plan_create || !ks265_tonemap_plan_destroy || !ks265_input_tonemap_validate || !ks265_input_tonemap) {
        if (!t->tm_warned) logf_(2, e0->log_level, "ks265enc: tone mapping is unavailable: the device library has no ks265_input_tonemap\n");
        t->tm_warned = 1;
        return QY_NOTSUPPORTED;
    }
    if (!e0->dev_in_on || e0->tm_on) return QY_NOTSUPPORTED;             /* behind ks265_enc_enable_device_input, once */
    for (int i = 0; i < t->nlanes; ++i) if (t->lane[i]->in_disp) return QY_NOTSUPPORTED;   /* after the first picture */
    if ((e0->W & 7) || (e0->H & 7) || e0->ragged) return QY_NOTSUPPORTED;  /* a ragged handle takes 8-bit I420 and NV12 only */
    const ks265_tonemap_cfg cfg = {tm->transfer, tm->curve, tm->full_range, tm->peak_nits == 0.0 ? 1000.0 : tm->peak_nits, tm->white_nits == 0.0 ? 203.0 : tm->white_nits};
    if (!ks265_tm_cfg_ok(cfg.transfer, cfg.curve, cfg.peak_nits, cfg.white_nits) || (cfg.full_range != 0 && cfg.full_range != 1)) return QY_NOTSUPPORTED;
    for (int i = 0; i < t->nlanes; ++i) {
        const int r = ks265_tonemap_plan_create(main_ctx(t->lane[i]), &cfg, &t->lane[i]->tm_plan);
        if (r) { for (int k = 0; k < i; ++k) { (void)ks265_tonemap_plan_destroy(main_ctx(t->lane[k]), t->lane[k]->tm_plan); t->lane[k]->tm_plan = NULL; } return hip_rc(r); }
    }
    for (int i = 0; i < t->nlanes; ++i) t->lane[i]->tm_on = 1;
    return QY_OK;
}

int ks265_enc_set_next_roi(void *h, const ks265_roi *roi)
{
    Top *t = (Top *)h;
    if (!t) return QY_POINTER;
    t->roi_set = 0;                                                     /* withdrawn; on any refusal below nothing is pending */
    if (!roi) return QY_OK;
    Enc *e0 = t->lane[0];
    if (!e0->roi_on) return QY_NOTSUPPORTED;
    if (roi->device != -1 && roi->device != e0->dev_id) return QY_NOTSUPPORTED;
    if (ks265_roi_check(roi->type, roi->log2_block, roi->pitch, e0->srcW, e0->srcH)) return QY_NOTSUPPORTED;
    if (!roi->data) return QY_POINTER;
    if (roi->device >= 0) {                                             /* the whole map is checked before anything of it is enqueued */
        const ks265_roi_desc d = {roi->type, roi->log2_block, ks265_roi_map_cols(e0->srcW, roi->log2_block), ks265_roi_map_rows(e0->srcH, roi->log2_block), roi->data, roi->pitch};
        const int rv = ks265_roi_validate(main_ctx(e0), &d);
        if (rv) return hip_rc(rv);
    }
    t->roi = *roi; t->roi_set = 1;
    return QY_OK;
}

int ks265_enc_set_overlay(void *h, int slot, const ks265_overlay *ov)
{
    Top *t = (Top *)h;
    if (!t) return QY_POINTER;
    Enc *e0 = t->lane[0];
    if (!ks265_input_overlay || !ks265_input_overlay_validate) {
        if (!t->ov_warned) logf_(2, e0->log_level, "ks265enc: overlays are unavailable: the device library has no ks265_input_overlay\n");
        t->ov_warned = 1;
        return QY_NOTSUPPORTED;
    }
    if (slot < 0 || slot >= KS265_OV_SLOTS) return QY_NOTSUPPORTED;
    if (!ov) { overlay_drop(t, slot); return QY_OK; }
    for (int i = 0; i < t->nlanes; ++i) if (t->lane[i]->dev_id != e0->dev_id || t->lane[i]->use_graph) return QY_NOTSUPPORTED;   /* lanes on several GPUs; the graph experiment (a fixed launch sequence) */
    if ((ov->flags & ~KS265_OV_FORCED_ONLY) || (ov->rgb.device != -1 && ov->rgb.device != e0->dev_id)) return QY_NOTSUPPORTED;
    if (!ov->rgb.plane[0] || !ov->rgb.plane[1] || !ov->rgb.plane[2]) return QY_POINTER;
    struct OvSlot n = {.on = 1, .dev = ov->rgb.device >= 0, .forced_only = (ov->flags & KS265_OV_FORCED_ONLY) != 0, .stream = ov->rgb.stream};
    n.d = (ks265_overlay_desc){.rgb = {.format = ov->rgb.format, .width = ov->width, .height = ov->height, .plane = {ov->rgb.plane[0], ov->rgb.plane[1], ov->rgb.plane[2]}, .pitch = {ov->rgb.pitch[0]},
                                       .pixel_step = ov->rgb.pixel_step, .matrix = ov->rgb.matrix, .full_range = ov->rgb.full_range}, .alpha = ov->alpha, .x = ov->x, .y = ov->y, .opacity = ov->opacity};
    if (!n.dev) {
        /* host memory: the bytes between the lowest channel sample of pixel (0, 0) and the end of the highest one's last row go to the device as they lie, and the description
         * moves with them.  What is needed to size the copy is judged here; everything else by the device library, on the copy */
        const int es = ov->rgb.format == KS265_IN_RGB ? 1 : ov->rgb.format == KS265_IN_RGB_F32 ? 4 : ov->rgb.format == KS265_IN_RGB_F16 || ov->rgb.format == KS265_IN_RGB_BF16 ? 2 : 0;
        if (!es || ov->width < 2 || ov->height < 2 || ov->width > 8192 || ov->height > 8192 || ov->rgb.pixel_step < es || ov->rgb.pixel_step > 64) return QY_NOTSUPPORTED;
        if ((long long)ov->rgb.pitch[0] < (long long)ov->width * ov->rgb.pixel_step) return QY_POINTER;
        uintptr_t lo = (uintptr_t)ov->rgb.plane[0], hi = lo;
        const void *ch[4] = {ov->rgb.plane[0], ov->rgb.plane[1], ov->rgb.plane[2], ov->alpha};
        for (int k = 1; k < 4; ++k) if (ch[k]) { const uintptr_t q = (uintptr_t)ch[k]; lo = q < lo ? q : lo; hi = q > hi ? q : hi; }
        if (hi - lo > (uintptr_t)4 * (uintptr_t)ov->rgb.pitch[0] * (uintptr_t)ov->height) return QY_NOTSUPPORTED;   /* (the channels of ONE buffer: at most four planes apart - the copy takes everything between them) */
        const size_t nb = (size_t)(hi - lo) + (size_t)ov->rgb.pitch[0] * (size_t)(ov->height - 1) + (size_t)(ov->width - 1) * (size_t)ov->rgb.pixel_step + (size_t)es;
        const size_t skew = lo & 15;                                    /* the copy keeps the address modulo 16: element alignment and the kernel's choice of loads stay */
        int r = ks265_dev_malloc(main_ctx(e0), &n.own, nb + skew);
        if (!r) r = ks265_memcpy_h2d_sync(main_ctx(e0), (uint8_t *)n.own + skew, (const void *)lo, nb);
        if (r) { if (n.own) ks265_dev_free(main_ctx(e0), n.own); return hip_rc(r); }
        const uint8_t *base = (const uint8_t *)n.own + skew;
        for (int k = 0; k < 3; ++k) n.d.rgb.plane[k] = base + ((uintptr_t)ch[k] - lo);
        if (ov->alpha) n.d.alpha = base + ((uintptr_t)ov->alpha - lo);
    }
    int r = hip_rc(ks265_input_overlay_validate(main_ctx(e0), &n.d, 1, e0->W, e0->H, e0->srcW, e0->srcH));
    /* every input slot of every lane needs its twin: made here if the lane has none and no picture is in flight */
    for (int i = 0; i < t->nlanes && !r; ++i) {
        Enc *e = t->lane[i];
        if (!lane_twins_missing(e)) continue;
        if (!lane_idle(e)) { logf_(2, e->log_level, "ks265enc: the handle's first overlay needs a device twin for every input slot, and pictures are in flight: set it before the first picture, on a zero-latency handle, or after a flush\n"); r = QY_NOTSUPPORTED; }
        else r = lane_make_twins(e);
    }
    if (r) { if (n.own) ks265_dev_free(main_ctx(e0), n.own); return r; }
    overlay_drop(t, slot);
    t->ov[slot] = n; ++t->ov_n;
    return QY_OK;
}

int ks265_enc_device_recon_pending(void *h)
{
    const Top *t = (const Top *)h;
    return t && t->lane[0]->devrecon ? recon_list_pending(&t->handed) : 0;
}

int ks265_enc_get_device_recon(void *h, const ks265_dev_picture *dst, QY265Picture *info)
{
    Top *t = (Top *)h;
    if (!t || !dst) return QY_POINTER;
    if (!t->lane[0]->devrecon || dst->device != t->lane[0]->dev_id) return QY_NOTSUPPORTED;
    const ReconRef *ref = recon_list_front(&t->handed);
    if (!ref) return QY_FAIL;
    Enc *e = t->lane[ref->lane];
    struct ReconSlot *q = &e->rslot[ref->slot];
    /* the whole destination is checked before anything is enqueued: a refused one leaves the picture pending */
    ks265_in_desc d;
    dev_desc(e, dst, &d);
    int r = e->ctx_rec ? KS265_OK : ks265_create(&e->ctx_rec, e->dev_id);   /* (its own stream goes at once: ks265_set_stream below) */
    if (!r) r = ks265_set_stream(e->ctx_rec, dst->stream);
    if (!r) r = ks265_output_validate(e->ctx_rec, &d);
    if (r) return hip_rc(r);
    /* the conversion runs IN the caller's stream - behind everything enqueued there before the call, in front of everything enqueued after it - once that stream has waited for the
     * picture's pack; ev_read behind it is what the slot's next pack waits for */
    r = ks265_stream_wait_event(e->ctx_rec, q->ev_packed);
    /* a ragged lane: the window first, into the lane's scratch picture, in the same stream - which may be another stream than the last call's: this crop waits for the conversion that
     * read the scratch picture last (ev_crop), as the slot's next pack waits for ev_read */
    if (!r && e->ragged && e->crop_used) r = ks265_stream_wait_event(e->ctx_rec, e->ev_crop);
    if (!r && e->ragged) r = ks265_output_crop(e->ctx_rec, q->dev, e->W, e->H, e->srcW, e->srcH, e->crop_scr);
    if (!r) r = ks265_output_convert(e->ctx_rec, e->ragged ? e->crop_scr : q->dev, &d);
    if (!r && e->ragged) { r = ks265_event_record(e->ctx_rec, e->ev_crop); if (!r) e->crop_used = 1; }
    if (!r) r = ks265_event_record(e->ctx_rec, q->ev_read);
    if (!r) q->read_on = 1;                                             /* (read by the scheduler thread when it takes the slot again: after this call's successor released it, under mu) */
    if (r) return hip_rc(r);
    if (info) { info->iSliceType = ref->slice_type; info->poc = ref->poc; info->pts = ref->pts; info->dts = ref->pts; }
    recon_list_pop(&t->handed);
    return QY_OK;
}

int ks265_enc_device_analysis_pending(void *h)
{
    const Top *t = (const Top *)h;
    return t && t->lane[0]->analysis ? recon_list_pending_an(&t->handed) : 0;
}

int ks265_enc_get_device_analysis(void *h, const ks265_dev_analysis *dst, QY265Picture *info)
{
    Top *t = (Top *)h;
    if (!t || !dst) return QY_POINTER;
    if (!t->lane[0]->analysis || dst->device != t->lane[0]->dev_id) return QY_NOTSUPPORTED;
    const ReconRef *ref = recon_list_front_an(&t->handed);
    if (!ref) return QY_FAIL;
    Enc *e = t->lane[ref->lane];
    struct ReconSlot *q = &e->rslot[ref->slot];
    /* every wanted field is checked before anything is enqueued: a refused one leaves the picture pending */
    const ks265_analysis_desc d = {e->W, e->H, {dst->mv.data, dst->mv.pitch, dst->mv.plane}, {dst->ref.data, dst->ref.pitch, dst->ref.plane}, {dst->cu.data, dst->cu.pitch, dst->cu.plane},
                                   {dst->qp.data, dst->qp.pitch, dst->qp.plane}, {dst->sse.data, dst->sse.pitch, dst->sse.plane}};
    int r = e->ctx_rec ? KS265_OK : ks265_create(&e->ctx_rec, e->dev_id);   /* (the context the reconstructions' conversions run on, if any ran: the calling thread's alone) */
    if (!r) r = ks265_set_stream(e->ctx_rec, dst->stream);
    if (!r) r = ks265_analysis_validate(e->ctx_rec, &d);
    if (r) return r == KS265_NOTSUPPORTED ? QY_POINTER : hip_rc(r);         /* (a pitch or an address the field cannot have: a bad field like any other) */
    /* the export runs IN the caller's stream once that stream has waited for the picture's packs; ev_read_an behind it is what the block's next pack waits for */
    r = ks265_stream_wait_event(e->ctx_rec, q->ev_packed);
    if (!r) r = ks265_analysis_export(e->ctx_rec, q->an, &d);
    if (!r) r = ks265_event_record(e->ctx_rec, q->ev_read_an);
    if (!r) q->read_on_an = 1;                                          /* (read by the scheduler thread when it takes the slot again: after this call's successor released it, under mu) */
    if (r) return hip_rc(r);
    if (info) { info->iSliceType = ref->slice_type; info->poc = ref->poc; info->pts = ref->pts; info->dts = ref->pts; }
    recon_list_pop_an(&t->handed);
    return QY_OK;
}

int ks265_enc_set_recon_file(void *h, const char *path)
{
    Top *t = (Top *)h;
    if (!t || !path) return QY_POINTER;
    if (t->n_in) return QY_NOTSUPPORTED;
    for (int i = 1; i < t->nlanes; ++i) lane_close(t->lane[i], 0);     /* the dump is one file in display order: one lane */
    t->nlanes = 1;
    return lane_set_recon_file(t->lane[0], path);
}
