/* TEST INFRASTRUCTURE (tests/test_lane_open_cpu.py): opens the encoder host (ks265codec_amd/host/ks265_enc.c) on the device library's stand-in (tests/hip_stub.c) for no other purpose
 * than to look at what the open creates and what the close gives back.  A program of its own, so that it can be built with sanitizers and run as it is.
 *   lane_open_main trace W H [name value]...   one open: the stand-in's line per creating call (in call order), the host's log lines (`log: `, in their order), then `open: ...`
 *   lane_open_main walk  W H [name value]...   the k-th creating call fails, for every k of a plain open: the open fails with QY_OUTOFMEMORY or takes a designed fall-back, and
 *                                               after the close no object of the stand-in is alive (walk:i/n: only the k with k mod n = i, so that n processes share the walk)
 * name value: a QY265ConfigParse pair, or one of ks265_enc_set_default (md5, hash, ...); `rc` also takes a value the parser refuses, written into the field as an SDK caller can.
 * The configuration starts as -preset medium at default latency with `threads 4` (the start-up line names the thread count) and `log 0` (every line).  KS265_* variables act as always. */
#include "ks265_enc.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

void ks265_stub_open_trace(FILE *fp);
void ks265_stub_fail_at(long k);
long ks265_stub_creating_calls(void);
long ks265_stub_live(int kind);
static const char *const kKinds[5] = {"contexts", "frame objects", "events", "device blocks", "pinned blocks"};

static char *g_log; static size_t g_log_len;
static void collect(const char *msg)
{
    const size_t n = strlen(msg);
    char *p = (char *)realloc(g_log, g_log_len + n + 1);
    if (!p) return;
    g_log = p; memcpy(g_log + g_log_len, msg, n + 1); g_log_len += n;
}

static const char *err_name(int e)
{
    return e == QY_OK ? "QY_OK" : e == QY_FAIL ? "QY_FAIL" : e == QY_OUTOFMEMORY ? "QY_OUTOFMEMORY" : e == QY_POINTER ? "QY_POINTER" : e == QY_NOTSUPPORTED ? "QY_NOTSUPPORTED" : "?";
}

static int live_objects(const char *when)
{
    int bad = 0;
    for (int k = 0; k < 5; ++k) if (ks265_stub_live(k)) { printf("FAIL %s: %ld %s alive\n", when, ks265_stub_live(k), kKinds[k]); bad = 1; }
    return bad;
}

/* the designed fall-backs of a failed stream: the lookahead's and the uploads' streams that are created in front of the main context go on without (the lookahead's is tried again
 * where its objects are made).  In the plain trace those are the `create` lines with another `create` between them and the next frame object - the last one of such a run is the
 * context that frame object is made on */
static int optional_stream(char **line, long n, long k)
{
    if (strncmp(line[k], "create", 6)) return 0;
    long j = k + 1;
    while (j < n && !strncmp(line[j], "create", 6)) ++j;
    return j > k + 1 && j < n && !strncmp(line[j], "frame ", 6);
}

int main(int argc, char **argv)
{
    if (argc < 4 || (argc & 1) || (strcmp(argv[1], "trace") && strncmp(argv[1], "walk", 4))) { fprintf(stderr, "usage: lane_open_main trace|walk[:i/n] W H [name value]...\n"); return 2; }
    const int walk = !strncmp(argv[1], "walk", 4);
    long part = 0, parts = 1;
    if (walk && argv[1][4] && (sscanf(argv[1] + 4, ":%ld/%ld", &part, &parts) != 2 || parts < 1 || part < 0 || part >= parts)) return 2;
    QY265EncConfig cfg;
    QY265ConfigDefault(&cfg, QY265PRESET_MEDIUM, QY265TUNE_DEFAULT, QY265LATENCY_DEFAULT);
    cfg.picWidth = atoi(argv[2]); cfg.picHeight = atoi(argv[3]); cfg.threads = 4; cfg.logLevel = 0;
    for (int i = 4; i + 1 < argc; i += 2) {
        int r = QY265ConfigParse(&cfg, argv[i], argv[i + 1]);
        if (r == QY265_PARAM_BAD_NAME) r = ks265_enc_set_default(argv[i], atoi(argv[i + 1]));
        else if (r == QY265_PARAM_BAD_VALUE && !strcmp(argv[i], "rc")) { cfg.rc = atoi(argv[i + 1]); r = 0; }
        if (r) { fprintf(stderr, "%s %s: refused (%d)\n", argv[i], argv[i + 1], r); return 2; }
    }
    QY265SetLogPrintf(collect);
    FILE *tf = tmpfile();
    if (!tf) return 2;
    int err = 0;
    ks265_stub_fail_at(0);
    ks265_stub_open_trace(tf);
    void *h = QY265EncoderOpen(&cfg, &err);
    ks265_stub_open_trace(NULL);
    const long ncalls = ks265_stub_creating_calls();
    const int lanes = h ? ks265_enc_lanes(h) : 0;
    const size_t log_at_open = g_log_len;
    QY265EncoderClose(h);
    int bad = live_objects("after the plain open's close");
    /* the trace as lines */
    const long tsz = ftell(tf);
    char *text = (char *)calloc((size_t)tsz + 1, 1);
    rewind(tf);
    if (!text || fread(text, 1, (size_t)tsz, tf) != (size_t)tsz) return 2;
    fclose(tf);
    long nlines = 0;
    for (long i = 0; i < tsz; ++i) nlines += text[i] == '\n';
    char **line = (char **)calloc((size_t)nlines + 1, sizeof *line);
    if (!line) return 2;
    { long k = 0; char *p = text; while (k < nlines) { line[k++] = p; p = strchr(p, '\n'); *p++ = 0; } }
    if (!walk) {
        for (long k = 0; k < nlines; ++k) puts(line[k]);
        for (size_t i = 0; i < log_at_open; ) {                          /* the log lines up to the end of the open */
            const char *nl = (const char *)memchr(g_log + i, '\n', log_at_open - i);
            const size_t n = nl ? (size_t)(nl - (g_log + i)) : log_at_open - i;
            printf("log: %.*s\n", (int)n, g_log + i);
            i += n + 1;
        }
        if (h) printf("open: ok, %d lane(s), %ld creating calls\n", lanes, ncalls); else printf("open: error %s\n", err_name(err));
        return bad;
    }
    if (!h || nlines != ncalls) { printf("FAIL: the plain open: %s, %ld trace lines for %ld creating calls\n", err_name(err), nlines, ncalls); return 1; }
    long n_fail = 0, n_stream = 0, n_lanes = 0;
    for (long k = 1; k <= ncalls; ++k) {
        if (k % parts != part) continue;
        char when[64]; snprintf(when, sizeof when, "k = %ld (%s)", k, line[k - 1]);
        ks265_stub_fail_at(k);
        h = QY265EncoderOpen(&cfg, &err);
        ks265_stub_fail_at(0);
        if (!h) { ++n_fail; if (err != QY_OUTOFMEMORY) { printf("FAIL %s: the open failed with %s\n", when, err_name(err)); bad = 1; } }
        else if (ks265_enc_lanes(h) < lanes) ++n_lanes;                  /* a GOP lane behind the first could not be opened: the handle goes on with the lanes there are (QY265EncoderOpen) */
        else if (optional_stream(line, nlines, k - 1)) { ++n_stream; printf("k = %ld (%s): the open goes on without that stream\n", k, line[k - 1]); }
        else { printf("FAIL %s: the open succeeded\n", when); bad = 1; }
        QY265EncoderClose(h);
        bad |= live_objects(when);
    }
    printf("walk %ld/%ld: %ld creating calls; %ld opens failed with QY_OUTOFMEMORY, %ld went on without an optional stream, %ld with fewer lanes: %s\n", part, parts, ncalls, n_fail, n_stream, n_lanes, bad ? "FAIL" : "ok");
    free(line); free(text); free(g_log);
    return bad;
}
