/* ks265_recon.h — the bookkeeping of `devrecon` (include/ks265_enc.h: reconstructed pictures handed out in device memory), plain C, nothing of the device library:
 * which slot of a lane's pool of packed-I420 pictures is free, which travels with a picture through the lane's ring (and the handle's chunk stash), which lies with the
 * caller; and the handle's list of the reconstructions its last call handed out, oldest first.  The encoder host (ks265_enc.c) owns the memory and the events behind a
 * slot number and does the locking (a pool under its lane's mutex; the list belongs to the calling thread); tests/recon_pool_main.c drives this unit alone.
 *
 *   RS_FREE --recon_pool_take--> RS_PICTURE --recon_pool_hand_out--> RS_OUT --recon_pool_release--> RS_FREE
 *
 * take: the scheduler, when it submits a picture (-1: none free - it waits, as for ring space).  hand_out: the call that hands the picture's NAL units out; the slot
 * joins the list (recon_list_push) in the order of the NAL units.  release: the NEXT call on the handle, for every entry of the list, fetched or not (recon_list_clear).
 * Every transition checks the state it leaves: a slot is never taken twice, handed out twice or released while a picture still travels with it. */
#ifndef KS265_RECON_H
#define KS265_RECON_H
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

enum { RS_FREE = 0, RS_PICTURE = 1, RS_OUT = 2 };
#define RECON_POOL_MAX 512

typedef struct ReconPool {
    int n, nfree;
    unsigned char state[RECON_POOL_MAX];
    short free_slot[RECON_POOL_MAX];                        /* a stack: the slot released last is taken first (its memory is the warmest) */
} ReconPool;

static inline int recon_pool_init(ReconPool *p, int n)
{
    memset(p, 0, sizeof *p);
    if (n < 1 || n > RECON_POOL_MAX) return -1;
    p->n = p->nfree = n;
    for (int i = 0; i < n; ++i) p->free_slot[i] = (short)(n - 1 - i);   /* slot 0 first */
    return 0;
}
static inline int recon_pool_take(ReconPool *p)
{
    if (!p->nfree) return -1;
    const int s = p->free_slot[--p->nfree];
    p->state[s] = RS_PICTURE;
    return s;
}
static inline int recon_pool_hand_out(ReconPool *p, int s)
{
    if (s < 0 || s >= p->n || p->state[s] != RS_PICTURE) return -1;
    p->state[s] = RS_OUT;
    return 0;
}
static inline int recon_pool_release(ReconPool *p, int s)
{
    if (s < 0 || s >= p->n || p->state[s] != RS_OUT) return -1;
    p->state[s] = RS_FREE;
    p->free_slot[p->nfree++] = (short)s;
    return 0;
}
/* a picture that is given up before it was submitted (an enqueue failed): its slot goes straight back */
static inline int recon_pool_untake(ReconPool *p, int s)
{
    if (s < 0 || s >= p->n || p->state[s] != RS_PICTURE) return -1;
    p->state[s] = RS_FREE;
    p->free_slot[p->nfree++] = (short)s;
    return 0;
}

/* one reconstruction on its way to the caller: the lane whose pool holds it, its slot there, and what ks265_enc_get_device_recon reports about the picture */
typedef struct ReconRef { int lane, slot, poc, slice_type; long long pts; } ReconRef;
/* in hand-out order; [0, next) have been fetched, [next, n) are pending.  `analysis` (include/ks265_enc.h) hands a second thing out with every picture - the slot's analysis
 * block - which is fetched on its own: a second cursor, next_an, over the same entries; neither cursor knows of the other */
typedef struct ReconList { ReconRef *v; int n, cap, next, next_an; } ReconList;

static inline int recon_list_push(ReconList *l, const ReconRef *r)
{
    if (l->n == l->cap) {
        const int nc = l->cap ? 2 * l->cap : 64;
        ReconRef *nv = (ReconRef *)realloc(l->v, (size_t)nc * sizeof *nv);
        if (!nv) return -1;
        l->v = nv; l->cap = nc;
    }
    l->v[l->n++] = *r;
    return 0;
}
static inline int recon_list_pending(const ReconList *l) { return l->n - l->next; }
static inline const ReconRef *recon_list_front(const ReconList *l) { return l->next < l->n ? &l->v[l->next] : NULL; }   /* the oldest pending one */
static inline void recon_list_pop(ReconList *l) { if (l->next < l->n) ++l->next; }                                    /* ... has been fetched */
static inline void recon_list_clear(ReconList *l) { l->n = l->next = l->next_an = 0; }                                 /* (after every entry was released) */
/* the analyses of the same entries: pending, the oldest pending one, fetched */
static inline int recon_list_pending_an(const ReconList *l) { return l->n - l->next_an; }
static inline const ReconRef *recon_list_front_an(const ReconList *l) { return l->next_an < l->n ? &l->v[l->next_an] : NULL; }
static inline void recon_list_pop_an(ReconList *l) { if (l->next_an < l->n) ++l->next_an; }
static inline void recon_list_free(ReconList *l) { free(l->v); memset(l, 0, sizeof *l); }
/* src's entries behind dst's, src left empty (a stashed GOP goes out) */
static inline int recon_list_move(ReconList *dst, ReconList *src)
{
    for (int i = 0; i < src->n; ++i) if (recon_list_push(dst, &src->v[i])) return -1;
    recon_list_clear(src);
    return 0;
}

/* a ragged size's dump (-o / ks265_enc_set_recon_file): the top-left w x h of a packed I420 picture of cw x ch, packed - what a decoder writes for the stream's conformance window */
static inline void ks265_recon_crop(const uint8_t *src, int cw, int ch, int w, int h, uint8_t *dst)
{
    for (int p = 0; p < 3; ++p) {
        const int s = p ? 2 : 1;
        for (int y = 0; y < h / s; ++y) memcpy(dst + (size_t)y * (w / s), src + (size_t)y * (cw / s), (size_t)(w / s));
        src += (size_t)(cw / s) * (ch / s); dst += (size_t)(w / s) * (h / s);
    }
}

#endif
