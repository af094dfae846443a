/* The GOP planner of the encoder host (ks265codec_amd/host/ks265_gop.h) on its own: no threads, no device library, nothing else of the host (tests/test_gop_plan_cpu.py).
 *   gop_plan_main plan < script : plans a clip as the scheduler thread would and prints one line per planned picture.  The script:
 *       rules gop_b hier refs refs_b refs0 gpb fixqp lean_b mg_adapt
 *       pic key mini4 iper              the facts that travel with the next input picture (display indices count from 0)
 *       wake have flush gop_end         one wake-up of the scheduler: it plans unit after unit until the planner says wait
 *     then plans the clip again with everything visible at once (one wake-up: the last one's have and gop_end, flush) and fails unless that yields the same units
 *   gop_plan_main walk : the B pictures gop_plan() emits for (lo, hi) are gop_walk()'s - the same pictures, order, interval ends, is_ref - for every span 2 .. 8 as a pyramid and
 *     2 .. 17 as plain B pictures.  (The host's ct_structure() copies gop_walk()'s nodes field by field; tests/test_calc_frame_cost.py covers that composition.) */
#include "ks265_gop.h"
#include <stdio.h>
#include <stdlib.h>

#define MAX_PICS 4096
static struct { int key, mini4, iper; } g_in[MAX_PICS];
static int g_nin;

/* the scheduler's loop without its executor: plan until the planner waits; every unit goes to out[] */
static int run_wake(const GopRules *g, GopState *st, int *d, int have, int flush, int gop_end, GopUnit *out, int nout, int cap, int *wake_of, int wake)
{
    for (;;) {
        GopView v; memset(&v, 0, sizeof v);
        v.have = have; v.flush = flush; v.gop_end = gop_end;
        for (int k = 0; k < GOP_VIEW; ++k) {
            const int disp = *d + 1 + k;
            if (disp < 0 || disp >= have || disp >= g_nin) continue;
            v.at[k].present = 1; v.at[k].key = g_in[disp].key; v.at[k].mini4 = g_in[disp].mini4; v.at[k].iper = g_in[disp].iper;
        }
        if (nout >= cap) { fprintf(stderr, "too many units\n"); exit(1); }
        const GopState before = *st;
        const int what = gop_plan(g, st, &v, *d, &out[nout]);
        if (what == GOP_GONE) { fprintf(stderr, "the planner lost a picture behind %d\n", *d); exit(1); }
        if (what == GOP_WAIT) {
            if (memcmp(&before, st, sizeof before)) { fprintf(stderr, "a wait behind %d changed the planner's state\n", *d); exit(1); }
            return nout;
        }
        if (wake_of) wake_of[nout] = wake;
        *d = out[nout++].a;
    }
}

static void print_list(const char *name, const int *v, int n)
{
    printf(" %s=", name);
    for (int i = 0; i < n; ++i) printf(i ? ",%d" : "%d", v[i]);
}

static int cmd_plan(void)
{
    static GopUnit scripted[MAX_PICS], once[MAX_PICS];
    static int wake_of[MAX_PICS]; int nwake = 0;                       /* the wake-up (counted from 0) in which each unit was planned */
    GopRules g; memset(&g, 0, sizeof g);
    GopState st; memset(&st, 0, sizeof st); st.mg4_until = -1;
    int d = -1, ns = 0, have = 0, gop_end = -1;
    char word[16];
    while (scanf("%15s", word) == 1) {
        if (!strcmp(word, "rules")) { if (scanf("%d %d %d %d %d %d %d %d %d", &g.gop_b, &g.hier, &g.refs, &g.refs_b, &g.refs0, &g.gpb, &g.fixqp, &g.lean_b, &g.mg_adapt) != 9) return 2; }
        else if (!strcmp(word, "pic")) { if (g_nin >= MAX_PICS || scanf("%d %d %d", &g_in[g_nin].key, &g_in[g_nin].mini4, &g_in[g_nin].iper) != 3) return 2; ++g_nin; }
        else if (!strcmp(word, "wake")) {
            int flush;
            if (scanf("%d %d %d", &have, &flush, &gop_end) != 3 || have > g_nin) return 2;
            ns = run_wake(&g, &st, &d, have, flush, gop_end, scripted, ns, MAX_PICS, wake_of, nwake++);
        } else return 2;
    }
    for (int i = 0; i < ns; ++i)
        for (int k = 0; k < scripted[i].n; ++k) {
            const GopPic *p = &scripted[i].pic[k];
            printf("pic wake=%d disp=%d poc=%d kind=%c gpb=%d layer=%d is_ref=%d lean=%d key_headers=%d qp_off=%d", wake_of[i], p->disp, p->poc, p->kind, p->gpb, p->layer, p->is_ref, p->lean, p->key_headers, p->qp_off);
            print_list("l0", p->l0, p->nl0); print_list("l1", p->l1, p->nl1); print_list("keep", p->keep, p->nk);
            printf("\n");
        }
    /* the planner's waits must not change what is eventually planned */
    GopState st1; memset(&st1, 0, sizeof st1); st1.mg4_until = -1;
    int d1 = -1;
    const int n1 = run_wake(&g, &st1, &d1, have, 1, gop_end, once, 0, MAX_PICS, NULL, 0);
    if (n1 != ns || d1 != d) { fprintf(stderr, "arrival: %d units up to %d picture by picture, %d up to %d with the whole clip visible\n", ns, d, n1, d1); return 1; }
    for (int i = 0; i < ns; ++i)
        if (memcmp(&scripted[i], &once[i], sizeof scripted[i])) { fprintf(stderr, "arrival: unit %d (ends at %d / %d) differs\n", i, scripted[i].a, once[i].a); return 1; }
    printf("arrival: same %d units\n", ns);
    return 0;
}

static int cmd_walk(void)
{
    for (int hier = 0; hier <= 1; ++hier)
        for (int span = 2; span <= (hier ? 8 : GOP_MAX_B + 1); ++span)      /* (plain B pictures: up to the longest mini-GOP the host opens) */
            for (int lo = 0; lo <= 16; lo += 8) {
                const int hi = lo + span;
                GopNode node[GOP_VIEW];
                const int nb = gop_walk(lo, hi, hier, node);
                /* the planner's unit for the same pictures: a GOP that started at 0, the last anchor at lo, the clip ends at hi */
                const GopRules g = {.gop_b = span > 8 ? span - 1 : 7, .hier = hier, .refs = 1, .refs_b = 1, .refs0 = 1, .lean_b = 1};
                GopState st = {.gop_start = 0, .anc_hist = {lo}, .n_anc = 1, .mg4_until = -1};
                GopView v; memset(&v, 0, sizeof v);
                v.have = hi + 1; v.flush = 1; v.gop_end = -1;
                for (int k = 0; k < span; ++k) v.at[k].present = 1;
                GopUnit u;
                if (gop_plan(&g, &st, &v, lo, &u) != GOP_UNIT || u.key || u.a != hi || u.n != nb + 1 || nb != span - 1 || u.pic[0].disp != hi) { printf("walk: hier %d (%d, %d): unit of %d, walk of %d\n", hier, lo, hi, u.n, nb); return 1; }
                for (int i = 0; i < nb; ++i) {
                    const GopPic *p = &u.pic[i + 1];
                    if (p->disp != node[i].b || p->is_ref != node[i].is_ref || p->layer != node[i].layer || p->nl0 != 1 || p->nl1 != 1 || p->l0[0] != node[i].lo || p->l1[0] != node[i].hi) {
                        printf("walk: hier %d (%d, %d): picture %d is %d (%d, %d) ref %d, the walk says %d (%d, %d) ref %d\n", hier, lo, hi, i, p->disp, p->l0[0], p->l1[0], p->is_ref, node[i].b, node[i].lo, node[i].hi, node[i].is_ref);
                        return 1;
                    }
                    if (!hier || (span & (span - 1))) { if (node[i].b != lo + 1 + i || node[i].is_ref) { printf("walk: (%d, %d) is no pyramid, yet picture %d is %d\n", lo, hi, i, node[i].b); return 1; } }
                    else if (node[i].b * 2 != node[i].lo + node[i].hi) { printf("walk: %d is not the middle of (%d, %d)\n", node[i].b, node[i].lo, node[i].hi); return 1; }
                }
                printf("walk: hier %d span %d at %d:", hier, span, lo);
                for (int i = 0; i < nb; ++i) printf(" %d%s", node[i].b - lo, node[i].is_ref ? "r" : "");
                printf("\n");
            }
    printf("walk: ok\n");
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 2 && !strcmp(argv[1], "plan")) return cmd_plan();
    if (argc == 2 && !strcmp(argv[1], "walk")) return cmd_walk();
    fprintf(stderr, "usage: %s plan < script | walk\n", argv[0]);
    return 2;
}
