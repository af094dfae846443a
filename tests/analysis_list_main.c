/* TEST INFRASTRUCTURE: drives the bookkeeping that `devrecon` and `analysis` share (ks265codec_amd/host/ks265_recon.h) with BOTH fetch cursors of the handle's list in use -
 * random submit / finish / stash / hand-out / fetch-a-reconstruction / fetch-an-analysis / release sequences over several lanes' pools and one handle's list, against a model
 * kept in plain arrays.  What it holds: each cursor walks the same entries in hand-out order and neither moves the other; a stashed GOP that goes out joins behind what is
 * pending for either cursor; the next call's release takes every slot back whatever either cursor has fetched, and leaves both cursors at the start of an empty list.  Built with
 * -fsanitize=address,undefined and run as a child process by tests/test_analysis_host_cpu.py.  argv: seed, steps.  Prints `ok <takes> <hand-outs> <recon fetches>
 * <analysis fetches> <releases>` or the first disagreement, exit status 1. */
#include "ks265_recon.h"
#include <stdio.h>

#define LANES 3
#define FAIL(...) do { printf(__VA_ARGS__); printf("\n"); return 1; } while (0)

static unsigned long long g_s;
static unsigned rnd(unsigned n) { g_s = g_s * 6364136223846793005ULL + 1442695040888963407ULL; return (unsigned)(g_s >> 33) % n; }

int main(int argc, char **argv)
{
    g_s = argc > 1 ? strtoull(argv[1], NULL, 10) : 1;
    const long steps = argc > 2 ? atol(argv[2]) : 100000;
    ReconPool pool[LANES]; ReconList handed = {0}, stash[LANES] = {{0}};
    int size[LANES];
    /* the model: every slot's state, every lane's pictures in flight (their slots, submission order), the handed-out (lane, slot, poc) in order, and how far each cursor is */
    static int m_state[LANES][RECON_POOL_MAX], m_fly[LANES][RECON_POOL_MAX], m_nfly[LANES], m_out[LANES * RECON_POOL_MAX][3], m_nout, m_next_rec, m_next_an;
    static int m_stash[LANES][RECON_POOL_MAX][2], m_nstash[LANES];
    long takes = 0, outs = 0, fetch_rec = 0, fetch_an = 0, releases = 0, poc = 0;
    for (int l = 0; l < LANES; ++l) { size[l] = 1 + (int)rnd(l == 0 ? 4 : 40); if (recon_pool_init(&pool[l], size[l])) FAIL("init"); }
    for (long s = 0; s < steps; ++s) {
        const int l = (int)rnd(LANES);
        switch (rnd(9)) {
        case 0: case 1: {                                              /* the scheduler submits a picture: one slot, whichever of the two switches is on */
            const int got = recon_pool_take(&pool[l]);
            if (got < 0) break;
            if (got >= size[l] || m_state[l][got] != RS_FREE) FAIL("step %ld: take gave %d", s, got);
            m_state[l][got] = RS_PICTURE; m_fly[l][m_nfly[l]++] = got; ++takes;
            break; }
        case 2: {                                                      /* the lane's oldest picture is finished: handed out directly, or stashed */
            if (!m_nfly[l]) break;
            const int slot = m_fly[l][0];
            memmove(m_fly[l], m_fly[l] + 1, (size_t)--m_nfly[l] * sizeof(int));
            const ReconRef ref = {l, slot, (int)poc, (int)rnd(3), 1000 + poc};
            if (rnd(2)) {
                if (recon_list_push(&stash[l], &ref)) FAIL("push");
                m_stash[l][m_nstash[l]][0] = slot; m_stash[l][m_nstash[l]++][1] = (int)poc;
            } else {
                if (recon_pool_hand_out(&pool[l], slot) || recon_list_push(&handed, &ref)) FAIL("step %ld: hand-out of slot %d refused", s, slot);
                m_state[l][slot] = RS_OUT; m_out[m_nout][0] = l; m_out[m_nout][1] = slot; m_out[m_nout++][2] = (int)poc; ++outs;
            }
            ++poc;
            break; }
        case 3: {                                                      /* a stashed GOP goes out: behind what either cursor still has pending */
            if (stash[l].next || stash[l].next_an) FAIL("step %ld: a stash with a moved cursor", s);
            for (int i = 0; i < m_nstash[l]; ++i) {
                if (recon_pool_hand_out(&pool[l], m_stash[l][i][0])) FAIL("step %ld: stashed slot refused", s);
                m_state[l][m_stash[l][i][0]] = RS_OUT; m_out[m_nout][0] = l; m_out[m_nout][1] = m_stash[l][i][0]; m_out[m_nout++][2] = m_stash[l][i][1]; ++outs;
            }
            if (stash[l].n != m_nstash[l] || recon_list_move(&handed, &stash[l]) || stash[l].n) FAIL("step %ld: move", s);
            m_nstash[l] = 0;
            break; }
        case 4: case 5: {                                              /* the caller fetches the oldest pending reconstruction */
            const int an_before = recon_list_pending_an(&handed);
            const ReconRef *f = recon_list_front(&handed);
            if (recon_list_pending(&handed) != m_nout - m_next_rec) FAIL("step %ld: reconstructions pending %d, model %d", s, recon_list_pending(&handed), m_nout - m_next_rec);
            if (m_next_rec == m_nout) { if (f) FAIL("step %ld: a reconstruction out of an empty list", s); recon_list_pop(&handed); }
            else {
                if (!f || f->lane != m_out[m_next_rec][0] || f->slot != m_out[m_next_rec][1] || f->poc != m_out[m_next_rec][2]) FAIL("step %ld: reconstruction fetch order", s);
                if (pool[f->lane].state[f->slot] != RS_OUT) FAIL("step %ld: a fetched slot is not out", s);
                recon_list_pop(&handed); ++m_next_rec; ++fetch_rec;
            }
            if (recon_list_pending_an(&handed) != an_before) FAIL("step %ld: a reconstruction's fetch moved the analyses' cursor", s);
            break; }
        case 6: case 7: {                                              /* ... the oldest pending analysis */
            const int rec_before = recon_list_pending(&handed);
            const ReconRef *f = recon_list_front_an(&handed);
            if (recon_list_pending_an(&handed) != m_nout - m_next_an) FAIL("step %ld: analyses pending %d, model %d", s, recon_list_pending_an(&handed), m_nout - m_next_an);
            if (m_next_an == m_nout) { if (f) FAIL("step %ld: an analysis out of an empty list", s); recon_list_pop_an(&handed); }
            else {
                if (!f || f->lane != m_out[m_next_an][0] || f->slot != m_out[m_next_an][1] || f->poc != m_out[m_next_an][2]) FAIL("step %ld: analysis fetch order", s);
                if (pool[f->lane].state[f->slot] != RS_OUT) FAIL("step %ld: a fetched slot is not out", s);
                recon_list_pop_an(&handed); ++m_next_an; ++fetch_an;
            }
            if (recon_list_pending(&handed) != rec_before) FAIL("step %ld: an analysis's fetch moved the reconstructions' cursor", s);
            break; }
        default: {                                                     /* the next call: every handed-out slot goes back, whatever was fetched of it */
            if (handed.n != m_nout) FAIL("step %ld: list %d, model %d", s, handed.n, m_nout);
            for (int i = 0; i < handed.n; ++i) {
                const ReconRef *r = &handed.v[i];
                if (recon_pool_release(&pool[r->lane], r->slot)) FAIL("step %ld: release refused", s);
                if (!recon_pool_release(&pool[r->lane], r->slot)) FAIL("step %ld: released twice", s);
                m_state[r->lane][r->slot] = RS_FREE; ++releases;
            }
            recon_list_clear(&handed); m_nout = m_next_rec = m_next_an = 0;
            if (recon_list_pending(&handed) || recon_list_pending_an(&handed) || recon_list_front(&handed) || recon_list_front_an(&handed)) FAIL("step %ld: a cleared list with something pending", s);
            break; }
        }
        for (int k = 0; k < LANES; ++k) {                              /* the books agree after every step */
            int nfree = 0;
            for (int i = 0; i < size[k]; ++i) { if (pool[k].state[i] != m_state[k][i]) FAIL("step %ld: lane %d slot %d state %d, model %d", s, k, i, pool[k].state[i], m_state[k][i]); nfree += m_state[k][i] == RS_FREE; }
            if (pool[k].nfree != nfree) FAIL("step %ld: lane %d free %d, model %d", s, k, pool[k].nfree, nfree);
        }
    }
    for (int l = 0; l < LANES; ++l) recon_list_free(&stash[l]);
    recon_list_free(&handed);
    printf("ok %ld %ld %ld %ld %ld\n", takes, outs, fetch_rec, fetch_an, releases);
    return 0;
}
