/* TEST INFRASTRUCTURE: drives the bookkeeping of `devrecon` (ks265codec_amd/host/ks265_recon.h) alone - random submit / finish / hand-out / fetch / release sequences over
 * several lanes' pools and one handle's list, against a model kept in plain arrays.  Built with -fsanitize=address,undefined and run as a child process by
 * tests/test_device_recon_host_cpu.py.  argv: seed, steps.  Prints `ok <takes> <hand-outs> <fetches> <releases> <refusals>` or the first disagreement, exit status 1. */
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
    /* the model: every slot's state, every lane's pictures in flight in submission order (their slots), the handed-out slots in order and how many were fetched */
    static int m_state[LANES][RECON_POOL_MAX], m_fly[LANES][RECON_POOL_MAX], m_nfly[LANES], m_out[LANES * RECON_POOL_MAX][2], m_nout, m_next, m_stash[LANES][RECON_POOL_MAX], m_nstash[LANES];
    long takes = 0, outs = 0, fetches = 0, releases = 0, refusals = 0, poc = 0;
    if (!recon_pool_init(&pool[0], 0) || !recon_pool_init(&pool[0], RECON_POOL_MAX + 1)) FAIL("a pool of no slots / of too many was accepted");
    for (int l = 0; l < LANES; ++l) { size[l] = 1 + (int)rnd(l == 0 ? 4 : 40); if (recon_pool_init(&pool[l], size[l])) FAIL("init"); }
    for (long s = 0; s < steps; ++s) {
        const int l = (int)rnd(LANES);
        switch (rnd(7)) {
        case 0: case 1: {                                              /* the scheduler submits a picture */
            int nfree = 0;
            for (int i = 0; i < size[l]; ++i) nfree += m_state[l][i] == RS_FREE;
            const int got = recon_pool_take(&pool[l]);
            if (!nfree) { if (got >= 0) FAIL("step %ld: a slot of a full pool", s); ++refusals; break; }
            if (got < 0 || got >= size[l] || m_state[l][got] != RS_FREE) FAIL("step %ld: take gave %d", s, got);
            m_state[l][got] = RS_PICTURE; m_fly[l][m_nfly[l]++] = got; ++takes;
            break; }
        case 2: {                                                      /* the oldest picture of the lane is finished: handed out directly, or (half of the time) stashed */
            if (!m_nfly[l]) break;
            const int slot = m_fly[l][0];
            memmove(m_fly[l], m_fly[l] + 1, (size_t)--m_nfly[l] * sizeof(int));
            const ReconRef ref = {l, slot, (int)poc++, (int)rnd(3), 1000 + poc};
            if (rnd(2)) {
                if (recon_list_push(&stash[l], &ref)) FAIL("push");
                m_stash[l][m_nstash[l]++] = slot;
            } else {
                if (recon_pool_hand_out(&pool[l], slot) || recon_list_push(&handed, &ref)) FAIL("step %ld: hand-out of slot %d refused", s, slot);
                if (!recon_pool_hand_out(&pool[l], slot)) FAIL("step %ld: slot %d handed out twice", s, slot);
                m_state[l][slot] = RS_OUT; m_out[m_nout][0] = l; m_out[m_nout++][1] = slot; ++outs;
            }
            break; }
        case 3: {                                                      /* a stashed GOP goes out */
            for (int i = 0; i < m_nstash[l]; ++i) {
                if (recon_pool_hand_out(&pool[l], m_stash[l][i])) FAIL("step %ld: stashed slot refused", s);
                m_state[l][m_stash[l][i]] = RS_OUT; m_out[m_nout][0] = l; m_out[m_nout++][1] = m_stash[l][i]; ++outs;
            }
            if (stash[l].n != m_nstash[l] || recon_list_move(&handed, &stash[l]) || stash[l].n) FAIL("step %ld: move", s);
            m_nstash[l] = 0;
            break; }
        case 4: case 5: {                                              /* the caller fetches the oldest pending one */
            const ReconRef *f = recon_list_front(&handed);
            if (recon_list_pending(&handed) != m_nout - m_next) FAIL("step %ld: pending %d, model %d", s, recon_list_pending(&handed), m_nout - m_next);
            if (m_next == m_nout) { if (f) FAIL("step %ld: a picture out of an empty list", s); recon_list_pop(&handed); break; }
            if (!f || f->lane != m_out[m_next][0] || f->slot != m_out[m_next][1]) FAIL("step %ld: fetch order", s);
            if (pool[f->lane].state[f->slot] != RS_OUT) FAIL("step %ld: a fetched slot is not out", s);
            recon_list_pop(&handed); ++m_next; ++fetches;
            break; }
        default: {                                                     /* the next call: every handed-out slot goes back, fetched or not */
            if (handed.n != m_nout) FAIL("step %ld: list %d, model %d", s, handed.n, m_nout);
            for (int i = 0; i < handed.n; ++i) {
                const ReconRef *r = &handed.v[i];
                if (recon_pool_release(&pool[r->lane], r->slot)) FAIL("step %ld: release refused", s);
                if (!recon_pool_release(&pool[r->lane], r->slot)) FAIL("step %ld: released twice", s);
                m_state[r->lane][r->slot] = RS_FREE; ++releases;
            }
            recon_list_clear(&handed); m_nout = m_next = 0;
            if (m_nfly[l] && !recon_pool_release(&pool[l], m_fly[l][0])) FAIL("step %ld: a slot in flight was released", s);
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
    printf("ok %ld %ld %ld %ld %ld\n", takes, outs, fetches, releases, refusals);
    return 0;
}
