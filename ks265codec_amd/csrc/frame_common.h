// frame_common.h — whole-frame stage plumbing shared by frame_*.hip (not part of the C ABI)
#pragma once
#include "ks265_internal.h"

#define KS_PAD_Y 80
#define KS_PAD_C 40
#define KS_COST_INVALID 0xFFFFFFFFu
#define KS_SAO_WS_WORDS 320            // cfg.sao == 3: words per CTU of ks265_frame::sao_ws
#define KS_SAO_CHAIN_ROWS 136          // ... and the CTU rows its merge chain keeps a diagonal's records in LDS for (pictures up to 8704 rows of samples)
#define KS_NSTAGE 8                   // me_integer, me_subpel, intra_candidates, cu_decide (+ merge pass), reconstruct, intra_pass, deblock, sao (+ padding)

// geometry handed to kernels by value
// cfg.part: what a CU of 64 / 32 / 16 samples costs in two halves (ks265_rect_decide): [0] = 2NxN (top, bottom), [1] = Nx2N (left, right); cost KS_COST_INVALID = not considered
struct KsRect { unsigned cost[2]; short mv[2][2][2]; short mv1[2][2][2]; unsigned char dir[2][2]; };   // B pictures: mv1 / dir = the half's list-1 vector and direction (ks265_cu_decide_part_b)

// Multi-reference B pictures (round 5; -preset veryslow = config 5: ref 4 / 4).  A block's pictures come from its record: inter_dir = direction | idx0 << 4 | idx1 << 6 (an
// index of a list the block does not use is 0: equal bytes = equal pictures, which is what the boundary strength compares).  Kernels pick a list's picture with selects - an
// indexed pointer array would lose the global address space.  idx0 / idx1: per PU record (85 per CTU) the picture ks265_ref_pick chose for the list; bits: lambda x ref_idx bits.
struct KsRefList { const uint8_t *p[4]; };
__device__ __forceinline__ const uint8_t *ks_pick(const KsRefList &r, int i) { return i == 0 ? r.p[0] : (i == 1 ? r.p[1] : (i == 2 ? r.p[2] : r.p[3])); }
struct KsMrefB { KsRefList y0, y1; const uint8_t *idx0, *idx1; int bits0[4], bits1[4]; };

struct KsGeom {
    int W, H;                 // luma size
    int sy, sc;               // strides
    long bytes_y, bytes_c;
    int ctu_cols, ctu_rows;
    int w8, h8;
    long org_y, org_c;        // byte offset of sample (0,0) inside a padded plane
};

// The searches of one picture that share their launches.  Every stage of the search chain - reference pyramid, pre-search, CTU order, integer search, propagation,
// sub-pel refinement - takes up to KS_BATCH_MAX searches of the same source picture in one grid: a work-group does for its search what it did when every search had launches
// of its own, the tails of the searches overlap inside the grid instead of following each other.  One entry = one search's operands; passed to the kernels by value.
#define KS_BATCH_MAX 4
#define KS_ME_ORDER_MAX 16384           // CTUs of a picture whose integer search is dispatched heavy-first (me_order_kernel keeps a score per CTU in LDS)
struct KsSearch {
    const uint8_t *ref;                 // the reference picture's luma plane (padded)
    uint8_t *r1, *r2, *r3;              // pre-search: its pyramid ...
    short2 *cand, *mv1, *ctu_off;       // ... the CTUs' votes, the L1 vectors (null: no pre-search), the CTUs' window offsets (null: zero)
    const ks265_pu *prev;               // temporal predictors (the nearest picture of a P picture; else null)
    ks265_pu *a, *b;                    // the integer search writes a; propagation round i reads a and writes b (i even) or the reverse; KsSearchBatch::final names the last one written
    const int *order; unsigned *work;   // heavy-first dispatch: this search's CTU order (null: the usual one) and the rounds it leaves behind (null: none)
};
struct KsSearchBatch { int n; KsSearch s[KS_BATCH_MAX]; };
// entry i with selects (i is uniform: scalar selects) - an indexed load from the by-value array would lose the pointers' global address space
__device__ __forceinline__ KsSearch ks_search_pick(const KsSearchBatch &B, int i)
{
    KsSearch s = B.s[0];
#pragma unroll
    for (int k = 1; k < KS_BATCH_MAX; ++k) {
        const bool t = i == k;
        s.ref = t ? B.s[k].ref : s.ref; s.r1 = t ? B.s[k].r1 : s.r1; s.r2 = t ? B.s[k].r2 : s.r2; s.r3 = t ? B.s[k].r3 : s.r3;
        s.cand = t ? B.s[k].cand : s.cand; s.mv1 = t ? B.s[k].mv1 : s.mv1; s.ctu_off = t ? B.s[k].ctu_off : s.ctu_off; s.prev = t ? B.s[k].prev : s.prev;
        s.a = t ? B.s[k].a : s.a; s.b = t ? B.s[k].b : s.b; s.order = t ? B.s[k].order : s.order; s.work = t ? B.s[k].work : s.work;
    }
    return s;
}
struct KsSearchWs { uint8_t *pyr[10]; ks265_pu *pu_s; unsigned *work; int *order; };

struct ks265_frame {
    ks265_ctx *ctx = nullptr;
    ks265_frame_cfg cfg{};
    ks265_frame_cfg cfg0{};             // the tools the frame object was created with (ks265_frame_set_picture_tools lowers and restores cfg's)
    ks265_frame_geom geom{};
    KsGeom g{};
    // workspace (device)
    // (no fractional planes: every consumer interpolates from the reference picture itself, interp_dev.h)
    ks265_pu *pu_x[3] = {nullptr, nullptr, nullptr};
    ks265_pu *pu1 = nullptr;
    ks265_pu_b *pub = nullptr;
    ks265_pu *pu[2] = {nullptr, nullptr};
    int cur_pu = 0;
    bool have_prev = false;
    ks265_cu8 *cu8 = nullptr;
    ks265_cu8 *cu8_tmp = nullptr;        // cfg.merge: the CU decision's map, input of the merge pass
    ks265_sao_param *sao = nullptr;
    int *sao_ws = nullptr;               // cfg.sao == 3: per CTU the statistics, own records and own cost the merge chain reads (KS_SAO_WS_WORDS words, frame_loop.hip)
    int16_t *lvl[3] = {nullptr, nullptr, nullptr};
    uint8_t *deb[3] = {nullptr, nullptr, nullptr};   // reconstructed picture before SAO (padded geometry)
    unsigned long long *sse = nullptr;
    unsigned long long *sse_acc = nullptr;   // ks265_sse_picture: three running sums + finished work-groups (zero between calls)
    unsigned long long *ssim_acc = nullptr;  // ks265_ssim_picture: [0..2] SSE sums, [3..5] fixed-point SSIM sums, [6] finished work-groups (zero between calls)
    unsigned *hash_acc = nullptr;            // ks265_picture_hash: [0..2] CRC parts, [3..5] checksums, [6] finished work-groups (zero between calls)
    short *mats = nullptr;              // forward + transposed DCT matrices of all sizes in the kernels' LDS layout (2 x MAT_SHORTS)
    int *progress = nullptr;            // intra wavefront: z-count per CTU (intra_deps.h), then the key pictures' CTU ticket
    const int8_t *qp_map = nullptr;      // round 4: one QP per CTU (ks265_frame_set_qp_map; null = cfg.qp everywhere), device memory of the host
    uint8_t *qp_eff = nullptr;           // ... and the QpY of every 8x8 block as the decoder derives it (deblocking), w8 * h8 bytes, allocated on first use
    void *rec_fence = nullptr;               // event the next picture waits for before it writes a record (ks265_frame_set_records_fence); consumed by that picture
    void *rect = nullptr;                                  // cfg.part: the 2NxN / Nx2N records of the P picture being coded (KsRect, 21 per CTU)
    int *ic_work = nullptr;                                // ... the CTUs that passed the candidates' gate: [0] = count, [4 ..] = CTU indices (round 5)
    uint32_t *icost = nullptr;                             // cfg.intra_inter: intra candidates of the P / B picture being coded (85 per CTU: cost << 6 | mode)
    // One workspace set per search of a picture that runs in the same launches (KsSearchBatch above): pyr = the pre-search's planes (cfg.pre_search): L1 / L2 of the source,
    // L1 / L2 of the reference, the CTUs' votes, L1 vectors, the 16x16 field, L3 of both, CTU window offsets - the source's [0] [1] [7] belong to set 0 and are shared by all;
    // pu_s = the other side of the propagation rounds (cfg.propagate); work / order = the heavy-first dispatch of the integer search (frame_me_int.hip me_order_kernel):
    // rounds per CTU wave of the set's previous search, the order built from them.  Set 0, and set 1 of a frame object made for B pictures, are allocated with the first
    // search; sets 2 and 3 when a picture first searches that many pictures at once (ks_search_ws)
    KsSearchWs ws[KS_BATCH_MAX] = {};
    int me_order_off = 0;               // KS265_ME_ORDER_OFF: experiments
    // cfg.rdoq (round 6; -rdoq 1 = the SDK's rdoq field, qy265enc.h:129): the luma transform blocks of inter CUs go through the reference's rdoQuant (rdoq_ops.hip) - front half of
    // ks265_reconstruct* (coefficients + levels rounded at 1 / 2 to planes), rdoq_prep_kernel (the blocks listed, packed, their significance masks and last positions), rdoq_kernel,
    // rdoq_unpack_kernel, back half (dequantisation, inverse transform, reconstruction).  Workspace allocated by ks265_frame_set_rdoq; tables + lambdas from the host per picture
    int16_t *rq_coef = nullptr, *rq_pack_lvl = nullptr, *rq_pack_coef = nullptr;
    ks265_rdoq_tu *rq_tus = nullptr;
    int *rq_pos = nullptr, *rq_ctr = nullptr, *rq_out = nullptr;
    int32_t *rq_tab = nullptr;
    long long *rq_lam = nullptr;
    uint16_t *rq_sigmask = nullptr;
    unsigned long long *rq_hidden = nullptr;
    bool rq_ready = false;
    uint8_t *ridx[2] = {nullptr, nullptr};              // multi-reference B pictures: per list the index of every PU's picture (ks265_ref_pick) ...
    ks265_pu *pu1_x[3] = {nullptr, nullptr, nullptr};   // ... and the records of list 1's pictures 1 .. refs - 1
    // optional in-situ stage timing (HIP events on the context's stream, between the stages of ks265_encode_picture)
    bool profiling = false;
    hipEvent_t ev[KS_NSTAGE + 1] = {};
    hipEvent_t ev_k[2] = {}; bool ev_k_valid = false;      // profiling: around the me_int_kernel launch alone (the SAD kernel of the roofline figure: stage me_integer also holds pre-search + propagation)
    int ev_k_n = 1;                                        // ... and the searches that launch carried (ks265_frame_me_int_ms reports the duration per search)
    bool ev_valid[KS_NSTAGE + 1] = {};
};

static inline ks265_pic ks_deb_pic(ks265_frame *f) { return ks265_pic{f->deb[0], f->deb[1], f->deb[2]}; }

// The pictures a picture predicts from.  The sequencer (frame_api.hip) builds the value once per picture and hands it to every stage that reads reference pictures; the
// exported stage functions build the one-picture-per-list value from their ref0 / ref1 arguments.  Nothing of it is kept on the frame object.
struct KsPicLists {
    int n[2];                 // pictures per list
    ks265_pic pic[2][4];      // entries past n repeat the list's last picture
    bool multi;               // a block's pictures come from its record (inter_dir = direction | idx0 << 4 | idx1 << 6): the multi-reference kernels
    bool pslice;              // two-list records, one list in the slice (multi-reference P picture): no list-1 prediction, the merge pass's zero candidate is uni-directional
};
static inline KsPicLists ks_pic_lists(const ks265_pic *refs0, int n0, const ks265_pic *refs1, int n1, bool multi, bool pslice)
{
    KsPicLists L{{n0, n1}, {}, multi, pslice};
    for (int i = 0; i < 4; ++i) { L.pic[0][i] = refs0[i < n0 ? i : n0 - 1]; L.pic[1][i] = refs1[i < n1 ? i : n1 - 1]; }
    return L;
}
static inline KsPicLists ks_pic_lists(ks265_pic ref0, ks265_pic ref1) { return ks_pic_lists(&ref0, 1, &ref1, 1, false, false); }   // one picture per list (ref1 = null picture: P)
// one plane (0: Y, 1: Cb, 2: Cr) of list l's pictures as a kernel argument (no list 1: its slots repeat list 0's pictures)
static inline KsRefList ks_ref_list(const KsPicLists &L, int l, int plane)
{
    KsRefList r;
    for (int i = 0; i < 4; ++i) {
        const ks265_pic p = L.pic[l][i].y ? L.pic[l][i] : L.pic[0][i];
        r.p[i] = plane == 0 ? p.y : plane == 1 ? p.u : p.v;
    }
    return r;
}

__device__ __forceinline__ const uint8_t *ks_org_y(const KsGeom &g, const uint8_t *p) { return p + g.org_y; }
__device__ __forceinline__ uint8_t *ks_org_y(const KsGeom &g, uint8_t *p) { return p + g.org_y; }
__device__ __forceinline__ const uint8_t *ks_org_c(const KsGeom &g, const uint8_t *p) { return p + g.org_c; }
__device__ __forceinline__ uint8_t *ks_org_c(const KsGeom &g, uint8_t *p) { return p + g.org_c; }

// PU indexing inside a CTU: level l (0: 64x64 .. 3: 8x8), raster
__device__ __forceinline__ int ks_level_base(int l) { return l == 0 ? 0 : l == 1 ? 1 : l == 2 ? 5 : 21; }
__device__ __forceinline__ int ks_pu_index(int l, int px, int py) { return ks_level_base(l) + py * (1 << l) + px; }
__device__ __forceinline__ bool ks_pu_inside(const KsGeom &g, int cx, int cy, int l, int px, int py)
{
    int s = 64 >> l, x0 = cx * 64 + px * s, y0 = cy * 64 + py * s;
    return x0 + s <= g.W && y0 + s <= g.H;
}

// XCD-aware block -> work-item map (cdna_hip_programming.md T1): block b runs on XCD b % 8; give every XCD a contiguous
// raster range of CTUs so that horizontally / vertically adjacent CTUs (which share reference rows and 128-byte lines)
// meet in the same 4 MiB L2.  Bijective for any n; speed only, never correctness.
__device__ __forceinline__ int ks_xcd_swizzle(int b, int n)
{
    const int per = n >> 3, rem = n & 7;                 // XCD x owns per + (x < rem) items
    const int x = b & 7, j = b >> 3;
    return x * per + min(x, rem) + j;
}

// legal vectors of the PUs of a CTU around its window offset (pre-search, else zero): +-range around the offset, and never so far that a block of the CTU
// leaves the 64-sample margin of the padded planes
__device__ __forceinline__ void ctu_mv_limits(const KsGeom &g, int range, int cx, int cy, int ox, int oy, int &lox, int &hix, int &loy, int &hiy)
{
    const int xe = min(cx * 64 + 64, g.W), ye = min(cy * 64 + 64, g.H);
    lox = max(ox - range, -64 - cx * 64); hix = min(ox + range, g.W + 64 - xe);
    loy = max(oy - range, -64 - cy * 64); hiy = min(oy + range, g.H + 64 - ye);
}

int ks265_frame_build_matrices(ks265_frame *f);      // frame_recon.hip
// the search chain on batches (frame_presearch.hip, frame_me_int.hip, frame_me.hip; no argument checks: the sequencer and the exported one-search functions made them)
int ks_search_ws(ks265_frame *f, int nsets, bool pyr);                          // workspace sets 0 .. nsets - 1 exist (allocated on first use; pyr: with the pre-search's planes)
KsSearch ks_search_entry(const ks265_frame *f, int set, ks265_pic ref, const ks265_pu *prev, ks265_pu *pu);   // one search on workspace set `set`, its records ending up in pu
int ks_presearch_source(ks265_frame *f, ks265_pic src);                         // the source picture's pyramid (once per picture)
int ks_presearch_batch(ks265_frame *f, const KsSearchBatch &B);                 // reference pyramids, L3 votes, window offsets, L2 / L1 vectors
int ks_me_integer_batch(ks265_frame *f, ks265_pic src, const KsSearchBatch &B); // CTU orders + the integer search
int ks_me_propagate_batch(ks265_frame *f, ks265_pic src, const KsSearchBatch &B, int round);
int ks_me_subpel_batch(ks265_frame *f, ks265_pic src, const KsSearchBatch &B, int final_b);   // final_b: the records are the entries' b (else a)
int ks265_sao_off(ks265_frame *f, ks265_sao_param *sao, ks265_pic dst);   // frame_loop.hip: the tail of a picture coded without SAO, in place
// the stages that read reference pictures, on explicit lists (the exported ks265_* functions of the same names wrap them; same argument checks)
int ks_bi_decide(ks265_frame *f, ks265_pic src, const KsPicLists &lists, const ks265_pu *pu0, const ks265_pu *pu1, ks265_pu_b *pub);                                         // frame_me.hip
int ks_bi_refine_chosen(ks265_frame *f, ks265_pic src, const KsPicLists &lists, const ks265_pu *pu0, const ks265_pu *pu1, ks265_pu_b *pub, ks265_cu8 *cu8);
int ks_cu_decide_part_b(ks265_frame *f, ks265_pic src, const KsPicLists &lists, const ks265_pu *pu0, const ks265_pu *pu1, const ks265_pu_b *pub, const uint32_t *ibest, ks265_cu8 *cu8);
int ks_merge_pass(ks265_frame *f, ks265_pic src, const KsPicLists &lists, const ks265_pu *pu, const ks265_pu_b *pub, const ks265_cu8 *cu_in, ks265_cu8 *cu_out);
int ks_skip_pass(ks265_frame *f, ks265_pic src, const KsPicLists &lists, ks265_cu8 *cu8, int16_t *lvl_y, int16_t *lvl_u, int16_t *lvl_v, ks265_pic recon);                  // frame_skip.hip
int ks_reconstruct(ks265_frame *f, ks265_pic src, const KsPicLists &lists, ks265_cu8 *cu8, int16_t *lvl_y, int16_t *lvl_u, int16_t *lvl_v, ks265_pic recon);                // frame_recon.hip (no checks: its callers made them)

// every frame-level entry point: the calling thread's current device is the frame's (a host with one encoder lane per GPU drives several devices from several
// threads; kernel launches go to the CURRENT device's streams only)
#define KS_FRAME_CHECK(f) do { if (!(f) || !(f)->ctx) return KS265_POINTER; ks_use_device((f)->ctx); } while (0)
