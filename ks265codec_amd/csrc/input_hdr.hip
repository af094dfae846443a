// input_hdr.hip — `vpp_hdr`: local contrast on the way in (tests/hdr_ref.py is the specification of every byte).  The luma of the packed I420 picture of
// W x H (multiples of 8) is smoothed by 2 or 3 iterations of the domain transform in its normalised-convolution form - a pass along the rows, then one along the columns -
// and the detail above that base is amplified IN PLACE.  Chroma is neither read nor written.  2 x iters launches on the context's stream, one per pass.
//
// What makes a pass exact and parallel at once: the window of a sample - every j of its line with |ct[j] - ct[x]| <= r - and the sum of J over it need only DIFFERENCES of
// the two running sums, so a work-group scans a piece of a line from wherever it likes.  d = 16 + slope |dY| is held to HDR_DMAX = 2481: a d above the largest radius ends
// every window that would cross it whatever its size, so the clamp changes no window, and the local ct stays below 2^21 where the reference needs 64 bits.
//
// A work-group of 256 threads owns 16 adjacent lines (rows for a row pass, columns for a column pass: a column strip is 16 samples = 8 dwords of J wide, lanes 0 .. 15 of
// a load or store run along the row) by up to 240 samples along the pass (1920 and 3840 are whole tiles):
//   staging   positions seg0 - halo - 1 .. seg0 + n + halo - 1 of every line, halo = r >> 4 <= 155 (d >= 16: no window reaches further), go to LDS as one dword
//             J | Y << 16 | inside << 24.  THE ADDRESS OF A POSITION OUTSIDE [0, N) OF THE LINE, OR OF A LINE OUTSIDE THE PLANE, IS REPLACED BY THAT OF THE PLANE'S FIRST
//             SAMPLE (the `inside` test in front of the address) and what the load brings is dropped: such a position stages 0.  A thread has 8 such loads in flight at a
//             time.  The first pass reads Y from the picture (J = 16 Y) and writes the guidance copy for its own samples;
//             every other pass reads that copy and a 16-bit plane.
//   scan      16 threads a line, a chunk of consecutive positions each (chunk odd: a wave's four chunks of a line start in different banks; lines lie at an odd pitch, so
//             the 16 lines of a lane group do too).  A thread reads its chunk once, keeps d | J << 12 in registers, sums them, the 16 totals of a line meet in LDS, and the
//             thread writes the inclusive sums over the staged dwords.  d of a position outside the line, and of the line's first sample, is HDR_DMAX: the picture's ends cut
//             the window with no special case in the search.
//   search    16 threads a line again, 15 consecutive samples each: the window's two ends of the first by binary search in ct over at most the halo, those of every
//             further sample by walking on from its neighbour's (both ends only ever move forward: ct rises), never past the halo; S and n from the sums, one rounded
//             division (on the float unit with one correcting step: the numerator is below 2^24, so exact).
//   output    a column pass stores as it goes - the 16 lanes of a lane group hold 16 adjacent columns of one row: 16-bit values to the other plane, or, in the LAST pass,
//             the boosted byte (Y from the copy) to the picture.  A row pass collects its tile in LDS and stores whole dwords along the rows.
// No pass reads neighbours from a plane it writes: picture -> A -> B -> A ... -> picture, the guidance from the copy.  dev_work = copy (W H bytes), A, B (2 W H each).
// Two builds of the kernel: halo <= 38 (radius <= 623: all of the default's passes, and the later iterations of most others) with 50 304 bytes of LDS, three work-groups
// on a CU's 160 KiB, and halo <= 155 with 80 256 bytes, two.  No scratch, no atomics.
#include "frame_common.h"

using namespace ks265;

namespace {

constexpr int HDR_LINES = 16, HDR_SEG = 240, HDR_HALO = 155, HDR_HALO_SMALL = 38, HDR_TPL = 256 / HDR_LINES;      // 16 threads a line
constexpr int HDR_DMAX = 2481, HDR_RMAX = 2480, HDR_BATCH = 8;

struct HdrArgs {
    const uint8_t *ysrc;          // the guidance: the picture (first pass) or the copy
    uint8_t *ycopy;               // first pass: the copy to write, else NULL
    const uint16_t *jin;          // NULL in the first pass
    uint16_t *jout;               // NULL in the last pass
    uint8_t *pic;                 // last pass: the luma to write
    int W, H, col, r, slope, gain;
};

template <int HALO>
struct HdrLds {
    static constexpr int LEN = HDR_SEG + 2 * HALO + 1;                  // staged positions of a line at most; odd: the pitch
    unsigned ct[HDR_LINES * LEN];
    unsigned sj[HDR_LINES * LEN];
    unsigned tct[256], tsj[256];
    uint16_t out[HDR_LINES * HDR_SEG];                                  // a row pass's tile on its way out
};

// num / den for num < 2^24 and 0 < den < 2^11, both exact as floats: the quotient of the fast division is at most one off, one step puts it right
__device__ __forceinline__ unsigned div_small(unsigned num, unsigned den)
{
    unsigned q = (unsigned)__fdividef((float)num, (float)den);
    const int rem = (int)(num - q * den);
    if (rem < 0) --q; else if (rem >= (int)den) ++q;
    return q;
}

template <int HALO>
__global__ __launch_bounds__(256) void input_hdr_pass_kernel(HdrArgs a)
{
    constexpr int LEN = HdrLds<HALO>::LEN;
    __shared__ __attribute__((aligned(16))) HdrLds<HALO> L;
    const int t = threadIdx.x;
    const int W = a.W, H = a.H;
    const int N = a.col ? H : W, NL = a.col ? W : H;                    // samples along a line, lines
    const int l0 = (a.col ? blockIdx.x : blockIdx.y) * HDR_LINES, seg0 = (a.col ? blockIdx.y : blockIdx.x) * HDR_SEG;
    const int n = min(HDR_SEG, N - seg0), halo = min(a.r >> 4, HALO), len = n + 2 * halo + 1, g0 = seg0 - halo - 1;
    const unsigned sl = a.col ? 1u : (unsigned)W, sp = a.col ? (unsigned)W : 1u;    // strides of a line and of a position (a sample's index is below 2^26: 32 bits do)
    // ---- staging: the lane index runs along the rows of the plane; HDR_BATCH loads of a thread are in flight together (a load outside the line or the plane is aimed
    //      at sample 0 of the plane and its value dropped)
    //      (l, p) of the thread's next dword are carried along: 256 dwords on are 256 / len lines and 256 % len positions on, no division per dword
    int sl_ = t & (HDR_LINES - 1), sp_ = t >> 4;
    if (!a.col) { sl_ = t / len; sp_ = t - sl_ * len; }
    else if (sp_ >= len) sl_ = HDR_LINES;                               // (a tile of fewer than 16 positions)
    const int dl = a.col ? 0 : 256 / len, dp = a.col ? 16 : 256 - dl * len;
    while (sl_ < HDR_LINES) {
        unsigned yv[HDR_BATCH], jv[HDR_BATCH];
        int lu[HDR_BATCH], pu[HDR_BATCH];
#pragma unroll
        for (int u = 0; u < HDR_BATCH; ++u) {
            lu[u] = sl_; pu[u] = sp_;
            sl_ += dl; sp_ += dp;
            if (!a.col && sp_ >= len) { sp_ -= len; ++sl_; }
            if (a.col && sp_ >= len) sl_ = HDR_LINES;
            const int g = g0 + pu[u];
            const bool inside = lu[u] < HDR_LINES && g >= 0 && g < N && l0 + lu[u] < NL;
            const unsigned at = inside ? (unsigned)(l0 + lu[u]) * sl + (unsigned)g * sp : 0u;
            yv[u] = a.ysrc[at] | (inside ? 1u << 8 : 0u);
            jv[u] = a.jin ? (unsigned)a.jin[at] : 16u * (yv[u] & 255u);
        }
#pragma unroll
        for (int u = 0; u < HDR_BATCH; ++u)
            if (lu[u] < HDR_LINES) {
                const bool inside = yv[u] >> 8;
                L.sj[lu[u] * LEN + pu[u]] = inside ? jv[u] | (yv[u] & 255u) << 16 | 1u << 24 : 0u;
                if (a.ycopy && inside && pu[u] > halo && pu[u] <= halo + n) a.ycopy[(unsigned)(l0 + lu[u]) * sl + (unsigned)(g0 + pu[u]) * sp] = (uint8_t)yv[u];
            }
    }
    __syncthreads();
    // ---- scan: thread (l, k) owns positions k chunk .. k chunk + chunk - 1 of line l, chunk <= CH, and reads them once: d | J << 12 stays in registers
    constexpr int CH = ((LEN + HDR_TPL - 1) / HDR_TPL) | 1;
    const int l = t & (HDR_LINES - 1), k = t >> 4, chunk = ((len + HDR_TPL - 1) / HDR_TPL) | 1;
    const int p0 = min(k * chunk, len), p1 = min(p0 + chunk, len);
    unsigned *sj = L.sj + l * LEN, *ct = L.ct + l * LEN;
    unsigned v[CH];
    unsigned prev = p0 > 0 && p0 < len ? sj[p0 - 1] : 0;               // the neighbour's last dword: read here, it is overwritten below
#pragma unroll
    for (int q = 0; q < CH; ++q) v[q] = p0 + q < p1 ? sj[p0 + q] : 0u;
    unsigned sd = 0, ss = 0;
#pragma unroll
    for (int q = 0; q < CH; ++q) {
        const int dy = abs((int)(v[q] >> 16 & 255u) - (int)(prev >> 16 & 255u));
        const unsigned d = (v[q] & prev) >> 24 ? (unsigned)min(HDR_DMAX, 16 + a.slope * dy) : (unsigned)HDR_DMAX, j = v[q] & 0xffffu;
        prev = v[q];
        v[q] = d | j << 12;
        if (p0 + q < p1) { sd += d; ss += j; }
    }
    L.tct[l * HDR_TPL + k] = sd; L.tsj[l * HDR_TPL + k] = ss;
    __syncthreads();
    sd = 0; ss = 0;
#pragma unroll
    for (int q = 0; q < HDR_TPL - 1; ++q) if (q < k) { sd += L.tct[l * HDR_TPL + q]; ss += L.tsj[l * HDR_TPL + q]; }
#pragma unroll
    for (int q = 0; q < CH; ++q)
        if (p0 + q < p1) { sd += v[q] & 4095u; ss += v[q] >> 12; ct[p0 + q] = sd; sj[p0 + q] = ss; }
    __syncthreads();
    // ---- search and output: thread (l, k) owns samples k xc .. k xc + xc - 1 of line l
    const int xc = (n + HDR_TPL - 1) / HDR_TPL, x0 = min(k * xc, n), x1 = min(x0 + xc, n);
    if (l0 + l < NL && x0 < x1) {
        const unsigned r = (unsigned)a.r;
        int p = halo + 1 + x0;
        unsigned cx = ct[p];
        int lo = p - halo, hi = p;                                      // the smallest j in [p - halo, p] with ct[p] - ct[j] <= r
        while (lo < hi) { const int m = (lo + hi) >> 1; if (cx - ct[m] <= r) hi = m; else lo = m + 1; }
        int top = p + halo;                                             // the largest j in [p, p + halo] with ct[j] - ct[p] <= r
        hi = p;
        while (hi < top) { const int m = (hi + top + 1) >> 1; if (ct[m] - cx <= r) hi = m; else top = m - 1; }
        for (int x = x0;;) {
            const unsigned S = sj[hi] - sj[lo - 1], cnt = (unsigned)(hi - lo + 1);
            const unsigned b = div_small(2u * S + cnt, 2u * cnt);
            if (!a.col) L.out[l * HDR_SEG + x] = (uint16_t)b;
            else {
                const unsigned at = (unsigned)(l0 + l) + (unsigned)(seg0 + x) * (unsigned)W;
                if (a.jout) a.jout[at] = (uint16_t)b;
                else {
                    const int y = a.ysrc[at], gd = a.gain * (16 * y - (int)b), m = (abs(gd) + 128) >> 8;
                    a.pic[at] = (uint8_t)min(255, max(0, gd < 0 ? y - m : y + m));
                }
            }
            if (++x == x1) break;
            cx = ct[++p];                                               // the next sample: both ends walk on, lo at most to p, hi at most to p + halo
            while (cx - ct[lo] > r) ++lo;
            hi = max(hi, p);
            while (hi < p + halo && ct[hi + 1] - cx <= r) ++hi;
        }
    }
    if (!a.col) {                                                       // (the same in every thread of the grid: the barrier is met by all)
        __syncthreads();
        const int nq = n >> 1;                                          // n is even: W is a multiple of 8, a tile begins at a multiple of 240
        const int ol = t >> 4;                                          // 16 lanes a row: 64 bytes a store
        if (l0 + ol < NL)
            for (int q = t & 15; q < nq; q += 16) *(unsigned *)(a.jout + (size_t)(l0 + ol) * W + seg0 + 2 * q) = *(const unsigned *)(L.out + ol * HDR_SEG + 2 * q);
    }
}

int hdr_check(ks265_ctx *c, const ks265_hdr_cfg *cfg, int w, int h)
{
    if (w <= 0 || h <= 0 || (w & 7) || (h & 7) || w > 8192 || h > 8192) { c->last_error = "hdr: width and height positive multiples of 8, at most 8192"; return KS265_NOTSUPPORTED; }
    bool ok = cfg->gain >= 1 && cfg->gain <= 80 && (cfg->iters == 2 || cfg->iters == 3) && cfg->slope >= 0 && cfg->slope <= 4096;
    for (int i = 0; ok && i < cfg->iters; ++i) ok = cfg->radius[i] >= 16 && cfg->radius[i] <= HDR_RMAX;
    if (!ok) { c->last_error = "hdr: gain 1 .. 80, iters 2 or 3, slope 0 .. 4096, every radius in use 16 .. 2480"; return KS265_NOTSUPPORTED; }
    return KS265_OK;
}

}  // namespace

extern "C" {

int ks265_input_hdr_validate(ks265_ctx *c, const ks265_hdr_cfg *cfg, int width, int height)
{
    if (!c || !cfg) return KS265_POINTER;
    return hdr_check(c, cfg, width, height);
}

size_t ks265_input_hdr_work_bytes(int width, int height)
{
    if (width <= 0 || height <= 0 || (width & 7) || (height & 7) || width > 8192 || height > 8192) return 0;
    return (size_t)5 * width * height;                                        // the guidance copy and the two 16-bit planes
}

int ks265_input_hdr(ks265_ctx *c, const ks265_hdr_cfg *cfg, int width, int height, uint8_t *dev_i420, void *dev_work, size_t work_bytes)
{
    if (!c || !cfg) return KS265_POINTER;
    ks_use_device(c);
    int r = hdr_check(c, cfg, width, height);
    if (r) return r;
    const long long npx = (long long)width * height, bytes = npx * 3 / 2, need = 5 * npx;
    uint8_t *work = (uint8_t *)dev_work;
    if (((uintptr_t)dev_i420 | (uintptr_t)work) & 3) { c->last_error = "hdr: the picture or the work buffer not 4-byte aligned"; return KS265_NOTSUPPORTED; }
    if (work_bytes < (size_t)need) { c->last_error = "hdr: the work buffer is smaller than ks265_input_hdr_work_bytes"; return KS265_POINTER; }
    if ((r = ks265_check_extent(c, dev_i420, bytes, 1, bytes, "picture"))) return r;
    if ((r = ks265_check_extent(c, work, need, 1, need, "work buffer"))) return r;
    if (work < dev_i420 + bytes && dev_i420 < work + need) { c->last_error = "hdr: the work buffer overlaps the picture"; return KS265_POINTER; }
    uint8_t *ycopy = work;
    uint16_t *plane[2] = {(uint16_t *)(work + npx), (uint16_t *)(work + 3 * npx)};
    const dim3 grid_row((unsigned)((width + HDR_SEG - 1) / HDR_SEG), (unsigned)((height + HDR_LINES - 1) / HDR_LINES));
    const dim3 grid_col((unsigned)((width + HDR_LINES - 1) / HDR_LINES), (unsigned)((height + HDR_SEG - 1) / HDR_SEG));
    const int passes = 2 * cfg->iters;
    for (int p = 0; p < passes && !r; ++p) {
        const bool first = p == 0, last = p == passes - 1;
        const HdrArgs a = {first ? dev_i420 : ycopy, first ? ycopy : nullptr, first ? nullptr : plane[(p + 1) & 1], last ? nullptr : plane[p & 1], dev_i420,
                           width, height, p & 1, cfg->radius[p >> 1], cfg->slope, cfg->gain};
        if ((a.r >> 4) <= HDR_HALO_SMALL) hipLaunchKernelGGL(input_hdr_pass_kernel<HDR_HALO_SMALL>, (p & 1) ? grid_col : grid_row, dim3(256), 0, c->stream, a);
        else hipLaunchKernelGGL(input_hdr_pass_kernel<HDR_HALO>, (p & 1) ? grid_col : grid_row, dim3(256), 0, c->stream, a);
        r = ks265_check_launch(c);
    }
    return r;
}

}  // extern "C"
