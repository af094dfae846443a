/* GOP planning: every GOP decision of the encoder host as a pure function of a handful of integers - which picture is a key picture, how long the mini-GOP is, coding order, slice
 * kinds, both reference lists, the reference picture sets, is_ref, the QP ladder.  No threads, no Enc, no device-library or stream-library call: ks265_enc.c gathers a view of its
 * input table, asks gop_plan() for the next unit and executes it (schedule); its cuTree pass walks the pictures of a mini-GOP with the same gop_walk() the planner uses.
 * Includable from anywhere (tests/gop_plan_main.c plans whole clips with nothing else of the host).  POCs are relative to the GOP's key picture. */
#ifndef KS265_GOP_H
#define KS265_GOP_H
#include <stdint.h>
#include <string.h>

/* the rules of a lane: what lane_resolve decided and the planner reads (filled once, behind lane_resolve) */
typedef struct GopRules {
    int gop_b, hier;                                      /* B pictures between two anchors; they form a pyramid (anchor distance 8 or 4) */
    int refs, refs_b, refs0;                              /* reference pictures of an IPPP picture / per list of a pyramid's B picture / past anchors an anchor of the pyramid searches */
    int gpb;                                              /* an anchor that searches two or more past anchors is coded as a B slice */
    int fixqp;                                            /* no QP ladder: every picture at the base QP */
    int lean_b;                                           /* KS265_LEAN_B: which B pictures run with fewer tools (GopPic::lean) */
    int mg_adapt;                                         /* slice-type decision: a block of 8 pictures is coded as 8 or as 4 + 4 (Input::mini4 of the block's last picture) */
} GopRules;

/* what the planner carries from one unit to the next */
typedef struct GopState {
    int gop_start;                                        /* display index of the last key picture */
    int anc_hist[4], n_anc;                               /* the last anchors' POCs, nearest first */
    int mg4_until;                                        /* display index up to which anchors are 4 apart (the second half of a block coded as 4 + 4) */
} GopState;

/* the input as one decision sees it: pictures [0, have) have arrived, flush = no more will come, a GOP ends at gop_end whatever follows (-1: none); at[k]: the picture with display
 * index d + 1 + k - the farthest a decision asks for is the anchor of the longest mini-GOP (gop_b + 1) or the d + 8 look of the slice-type decision.  GOP_MAX_B: the most B
 * pictures between two anchors (lane_open refuses more: under the caller's back-pressure, lane_put, a longer mini-GOP never arrives completely) */
#define GOP_MAX_B 16
#define GOP_VIEW (GOP_MAX_B + 1)
typedef struct GopView { int have, flush, gop_end; struct { int present, key, mini4, iper; } at[GOP_VIEW]; } GopView;

/* one planned picture */
typedef struct GopPic {
    int disp, poc, kind, gpb, layer;                      /* kind 'I' / 'P' / 'B'; gpb: kind 'P' with a list 1 - coded and signalled as a B picture, everything else treats it as the P picture it is; layer of the pyramid (0: anchors, plain B pictures) */
    int l0[4], nl0, l1[4], nl1;
    int keep[16], nk;                                     /* POCs that must stay in the DPB behind this picture: what later pictures still need, then list 0, then list 1 */
    int is_ref, key_headers;
    int lean;                                             /* 2: a B picture nothing predicts from; 1: a B picture others predict from whose own references are at most two pictures away; else 0 */
    int qp_off;                                           /* the QP ladder: this picture's offset on the base QP */
} GopPic;

/* a key picture alone, or a mini-GOP in coding order: its anchor, then its B pictures */
typedef struct GopUnit { int key, a, iper, n; GopPic pic[GOP_VIEW]; } GopUnit;   /* a: the unit's last display index; iper: the key period in force for it */

enum { GOP_WAIT, GOP_UNIT, GOP_GONE };                   /* nothing can be coded yet / one unit / a picture of the unit has left the input table (the encoder is being torn down) */

/* the QP ladders.  P pictures: + 1 on the key picture's; IPPP: the reference's own cascade over four pictures (appencoder -bframes 0 -qp 27 -psnr 2: 30 / 29 / 30 / 28 / 30 ..),
 * measured with the CPU mirror of the host: - 12 % bytes of the P pictures for - 0.09 dB */
static const int kIpppCascade[4] = {0, 2, 1, 2};
/* B pictures of the pyramid: + 2 / + 4 / + 4 on the key picture's QP by layer - the reference's own ladder (appencoder -qp 27 -psnr 2: anchors 28, B pictures 29 / 31 / 31; ours was
 * + 2 / + 3 / + 4 until the end of round 3).  Larger offsets keep paying (+ 3 / + 5 / + 6: 1.51 x -> 1.44 x the reference's bitrate at its PSNR-Y on the 1080p clip, every B picture within 0.1 dB
 * of the anchors - their quality comes from their references), but -qp would no longer mean what it means in the reference.  -bframes 3: + 2 / + 3
 * (the adaptive GOP's blocks of 4 keep + 2 / + 4: the reference's + 2 / + 3 there cost 1.3 % more bytes for + 0.004 dB on the 2160p clip, measured on the GPU at the end of round 4).
 * Plain B pictures: + 2, a rule of its own (gop_plan) */
static const int kHierLayerQp[4] = {0, 1, 3, 3}, kPyr4LayerQp[4] = {0, 1, 2, 2};

/* THE mini-GOP walk: the B pictures of (lo, hi) in coding order, each with the two pictures it lies between.  Pyramid (hier, a power of two apart): breadth first, every picture
 * in the middle of its interval, a reference where a half of that interval holds further pictures; else every picture between the two anchors, none of them a reference */
typedef struct GopNode { int b, lo, hi, is_ref, layer; } GopNode;
static int gop_walk(int lo, int hi, int hier, GopNode out[GOP_VIEW])
{
    int n = 0;
    if (!hier || ((hi - lo) & (hi - lo - 1)) != 0 || hi - lo > 8) {
        for (int b = lo + 1; b < hi && n < GOP_VIEW; ++b) out[n++] = (GopNode){b, lo, hi, 0, 0};
        return n;
    }
    struct { int lo, hi, layer; } q[16]; int head = 0, tail = 0;      /* intervals in the order they were made = layer by layer */
    q[tail].lo = lo; q[tail].hi = hi; q[tail++].layer = 1;
    for (; head < tail; ++head) {
        if (q[head].hi - q[head].lo < 2) continue;
        const int mid = (q[head].lo + q[head].hi) / 2;
        out[n++] = (GopNode){mid, q[head].lo, q[head].hi, (mid - q[head].lo >= 2) || (q[head].hi - mid >= 2), q[head].layer};
        q[tail].lo = q[head].lo; q[tail].hi = mid; q[tail++].layer = q[head].layer + 1;
        q[tail].lo = mid; q[tail].hi = q[head].hi; q[tail++].layer = q[head].layer + 1;
    }
    return n;
}

/* a planned picture is complete: its lists join its keep set, and what follows from its kind and lists */
static void gop_pic_finish(const GopRules *g, GopPic *p)
{
    for (int i = 0; i < p->nl0; ++i) p->keep[p->nk++] = p->l0[i];
    for (int i = 0; i < p->nl1; ++i) p->keep[p->nk++] = p->l1[i];
    p->gpb = p->kind == 'P' && p->nl1 > 0;
    /* round 6: a B picture nothing predicts from (half the pictures of a pyramid of 8) runs without intra candidates, without the joint refinement of its bi-predictive CUs and
     * without SAO - on the CPU mirror and on the MI355X its bytes at equal PSNR-Y stay (the refinement even costs bytes at QP + 4), a quarter of its kernel time goes
     * ... and a B picture others predict from whose own references are at most two pictures away (the second-deepest layer of a pyramid) keeps the refinement but runs without intra
     * candidates and without SAO: neutral at equal PSNR-Y on the mirror's three clips (profiles/r06_lean_b.txt).  KS265_LEAN_B=3: the non-reference pictures alone */
    const int near = p->kind == 'B' && p->is_ref && p->nl0 > 0 && p->nl1 > 0 && p->poc - p->l0[0] <= 2 && p->l1[0] - p->poc <= 2;
    p->lean = !g->lean_b || p->kind != 'B' ? 0 : !p->is_ref ? 2 : near && g->lean_b != 3 ? 1 : 0;
    if (g->fixqp) p->qp_off = 0;
}

/* the next unit behind display index d (= everything up to d is scheduled; -1 before the first picture).  GOP_WAIT leaves *st as it was; GOP_UNIT has advanced it - a caller that
 * may still decide to wait (the cuTree window) plans on a copy and keeps it once the unit is certain to be coded */
static int gop_plan(const GopRules *g, GopState *st, const GopView *v, int d, GopUnit *u)
{
    if (d + 1 >= v->have) return GOP_WAIT;
    const int nxt = d + 1;
    const int iper = v->at[0].present ? v->at[0].iper : 0;           /* the period in force when this picture was handed in (QY265EncoderReconfig) */
    memset(u, 0, sizeof *u);
    u->iper = iper;
    if (d < 0 || (iper > 0 && nxt - st->gop_start >= iper) || (v->at[0].present && v->at[0].key)) {
        if (!v->at[0].present) return GOP_GONE;
        st->gop_start = nxt; st->mg4_until = -1;
        st->anc_hist[0] = 0; st->n_anc = 1;                            /* the key picture is the GOP's first anchor (POC 0) */
        u->key = 1; u->a = nxt; u->n = 1;
        u->pic[0].disp = nxt; u->pic[0].kind = 'I'; u->pic[0].is_ref = 1; u->pic[0].key_headers = 1;
        return GOP_UNIT;
    }
    int span = g->gop_b + 1, mg4 = st->mg4_until;                      /* anchor distance */
    if (g->mg_adapt && span == 8) {                                    /* slice-type decision (lane_put): this block of 8 as two mini-GOPs of 4 */
        if (d < mg4) span = 4;                                         /* its second half */
        else if (d + 8 < v->have && v->at[7].present && v->at[7].mini4 && !v->at[7].key) { span = 4; mg4 = d + 8; }   /* the decision travels with the block's last picture; not there yet:
                                                                                                                       * nothing is coded before it arrives (or a key picture / the flush cuts the block short) */
    }
    int a = d + span;
    if (iper > 0 && a - st->gop_start >= iper) a = st->gop_start + iper - 1;   /* the mini-GOP in front of a key picture is shortened */
    for (int k = nxt + 1; k <= a && k < v->have; ++k)                   /* a picture asked to be a key picture: the mini-GOP in front of it is shortened as well */
        if (v->at[k - nxt].present && v->at[k - nxt].key) { a = k - 1; break; }
    if (v->gop_end >= nxt && a > v->gop_end) a = v->gop_end;            /* the GOP was closed behind this picture (its successor goes to another lane) */
    if (a >= v->have) { if (!v->flush) return GOP_WAIT; a = v->have - 1; }
    for (int k = nxt; k <= a; ++k) if (!v->at[k - nxt].present) return GOP_GONE;
    st->mg4_until = mg4;
    const int pd = d - st->gop_start, pa = a - st->gop_start;
    GopPic *p = &u->pic[u->n++];
    p->disp = a; p->poc = pa; p->kind = 'P'; p->is_ref = 1;
    p->qp_off = 1 + (g->gop_b == 0 ? kIpppCascade[pa & 3] : 0);
    if (span == 1) {                                                   /* IPPP: the most recent pictures, nearest first */
        for (int i = 0; i < g->refs && pa - 1 - i >= 0; ++i) p->l0[p->nl0++] = pa - 1 - i;
        for (int i = 0; i < g->refs - 1 && pa - 1 - i >= 0; ++i) p->keep[p->nk++] = pa - 1 - i;   /* still needed by the next picture */
    } else if (g->refs0 > 1 && st->n_anc > 0 && st->anc_hist[0] == pd) {
        /* -ref0: the last anchors of this GOP, nearest first (the first one is the previous anchor); all of them but the oldest are the next anchor's too */
        /* `gpb`: with two or more of them the anchor goes out as a B slice - the second nearest alone in list 1, the others in list 0: no picture in both lists (the boundary
         * strength compares list indices), bi-prediction pairs the two nearest anchors, every picture is searched once.  The pictures, and with them the reference picture
         * sets, are the P anchor's; the order is not the default construction's (8.3.4 gives both lists of past pictures the same order): list_mod */
        for (int i = 0; i < g->refs0 && i < st->n_anc; ++i) { if (g->gpb && i == 1) p->l1[p->nl1++] = st->anc_hist[i]; else p->l0[p->nl0++] = st->anc_hist[i]; }
        for (int i = 0; i < g->refs0 - 1 && i < st->n_anc; ++i) p->keep[p->nk++] = st->anc_hist[i];
    } else { p->l0[p->nl0++] = pd; p->keep[p->nk++] = pd; }
    gop_pic_finish(g, p);
    if (span > 1) {                                                    /* the anchors' history: this one in front */
        for (int i = 3; i > 0; --i) st->anc_hist[i] = st->anc_hist[i - 1];
        st->anc_hist[0] = pa; if (st->n_anc < 4) ++st->n_anc;
    }
    /* the B pictures.  A pyramid keeps every reference picture of the mini-GOP until its interval is done; simplest exact rule: all already coded reference pictures of [d, a]
     * (at most 5 with GOP 8).  -ref0: the anchors the NEXT anchor searches besides d and a stay in every B picture's set as well (they are in no list of it) */
    GopNode node[GOP_VIEW];
    const int nb = gop_walk(d, a, g->hier, node);
    int coded[8] = {pd, pa}, ncoded = 2;
    const int *lq = g->gop_b == 3 ? kPyr4LayerQp : kHierLayerQp;
    for (int i = 0; i < nb; ++i) {
        const int pm = node[i].b - st->gop_start;
        p = &u->pic[u->n++];
        p->disp = node[i].b; p->poc = pm; p->kind = 'B'; p->is_ref = node[i].is_ref; p->layer = node[i].layer;
        p->qp_off = p->layer ? 1 + lq[p->layer < 3 ? p->layer : 3] : 2;   /* (layer 0: plain B pictures) */
        for (int q = 0; q < ncoded; ++q) p->keep[p->nk++] = coded[q];
        for (int q = 2; q < g->refs0 && q < st->n_anc; ++q) p->keep[p->nk++] = st->anc_hist[q];
        /* list 0: the nearest pictures before this one among those the mini-GOP keeps, nearest first; list 1: those after it.  The interval's ends come first; -ref > 1 adds the
         * next nearest ones (plain B pictures keep nothing but the two anchors: those) */
        for (int want = 0; want < g->refs_b; ++want) {
            int b0 = -1000000, b1 = 1000000;
            for (int q = 0; q < ncoded; ++q) {
                if (coded[q] < pm && coded[q] > b0 && (p->nl0 == 0 || coded[q] < p->l0[p->nl0 - 1])) b0 = coded[q];
                if (coded[q] > pm && coded[q] < b1 && (p->nl1 == 0 || coded[q] > p->l1[p->nl1 - 1])) b1 = coded[q];
            }
            if (b0 > -1000000) p->l0[p->nl0++] = b0;
            if (b1 < 1000000) p->l1[p->nl1++] = b1;
        }
        gop_pic_finish(g, p);
        if (p->is_ref) coded[ncoded++] = pm;
    }
    u->a = a;
    return GOP_UNIT;
}
#endif
