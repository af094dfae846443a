// intra_deps.h — which neighbour CTUs an intra CU reads, and how far each of them must be coded first (the intra wavefront's one dependency rule).
// Plain C++ (host and device): frame_intra.hip waits on it, tests/test_intra_deps.py checks it against H.265 6.4.1 on the CPU.
//
// Progress of a CTU = its z-count: the number of its 8x8 blocks, in z-order, whose reconstructed samples are final and visible (0 .. 64; blocks
// outside the picture count as done).  Block b of CTU k is done exactly when progress[k] > z(b): blocks complete in z-order, so a CTU's right
// column completes top to bottom and its bottom row left to right.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define KS_HD __host__ __device__ __forceinline__
#else
#define KS_HD inline
#endif

namespace ks265 {

// z-order index of the 8x8 block (bx, by) of a CTU (bx, by in 0 .. 7)
KS_HD int ks_zorder(int bx, int by)
{
    const int sx = (bx & 1) | ((bx & 2) << 1) | ((bx & 4) << 2), sy = (by & 1) | ((by & 2) << 1) | ((by & 4) << 2);
    return sx | (sy << 1);
}

enum { KS_NBR_LEFT = 0, KS_NBR_TOPLEFT = 1, KS_NBR_TOP = 2, KS_NBR_TOPRIGHT = 3, KS_NBR_COUNT = 4 };

// The CU at block (lx, ly) of CTU (cx, cy), n8 x n8 blocks (n8 = 1, 2, 4), in a picture of w8 x h8 blocks and ctu_cols CTUs per row: the z-count
// that neighbour `which` must reach before the CU may read its samples, 0 = the CU reads nothing there.  *ctu = that neighbour's raster index.
// The samples an intra CU reads outside its own CTU (H.265 8.4.4.2.2, availability 6.4.1): the left column x0 - 1 from the corner down to the end
// of the below-left part (2 n rows below the corner, cut at the CTU row and the picture), in the left CTU when lx == 0; the row above from the corner
// to the end of the above-right part (x0 + 2 n - 1, cut at the picture), in the CTUs above when ly == 0.  Every one of them lies in a CTU with a
// smaller raster index (the below-left samples of the bottom CTU row inside the left CTU, the above-right ones in the row above), so all are
// available when inside the picture.  The furthest block read in a column / row has the highest z of those read there.
KS_HD int ks_intra_need(int which, int ctu_cols, int w8, int h8, int cx, int cy, int lx, int ly, int n8, int *ctu)
{
    *ctu = -1;
    if (which == KS_NBR_LEFT) {
        if (lx != 0 || cx == 0) return 0;
        int yb = ly + 2 * n8 - 1;                                          // the last row of the below-left part
        if (yb > 7) yb = 7;                                                // (below the CTU row: a later CTU, not available)
        if (yb > h8 - 1 - cy * 8) yb = h8 - 1 - cy * 8;                    // below the picture
        *ctu = cy * ctu_cols + cx - 1;
        return ks_zorder(7, yb) + 1;
    }
    if (ly != 0 || cy == 0) return 0;
    if (which == KS_NBR_TOPLEFT) {
        if (lx != 0 || cx == 0) return 0;
        *ctu = (cy - 1) * ctu_cols + cx - 1;
        return ks_zorder(7, 7) + 1;
    }
    if (which == KS_NBR_TOP) {
        int xb = lx + 2 * n8 - 1;                                          // the last column of the above-right part
        if (xb > 7) xb = 7;
        if (xb > w8 - 1 - cx * 8) xb = w8 - 1 - cx * 8;                    // right of the picture
        *ctu = (cy - 1) * ctu_cols + cx;
        return ks_zorder(xb, 7) + 1;
    }
    if (which == KS_NBR_TOPRIGHT) {
        if (lx + 2 * n8 <= 8 || cx + 1 >= ctu_cols) return 0;
        int xb = lx + 2 * n8 - 9;
        if (xb > w8 - 1 - (cx + 1) * 8) xb = w8 - 1 - (cx + 1) * 8;
        *ctu = (cy - 1) * ctu_cols + cx + 1;
        return ks_zorder(xb, 7) + 1;
    }
    return 0;
}

// Ticket t (0 .. ctu_cols * ctu_rows - 1) -> the raster index of the CTU coded t-th, in wavefront order: diagonal d = cx + 2 cy, the upper row first
// inside a diagonal.  Every CTU ks_intra_need returns lies on an earlier diagonal (left d - 1, top-left d - 3, top d - 2, top-right d - 1), so a CTU
// only ever waits for smaller tickets.  (Raster order hands the workers whole rows ahead of the wavefront: at 2160p a CTU waited for its left
// neighbour a third of a CTU per CTU along its row, and 128 workers held only two rows - 44 ms against 18.7 for one work-group per row.)
KS_HD int ks_ctu_of_ticket(int t, int ctu_cols, int ctu_rows)
{
    for (int d = 0;; ++d) {
        int lo = (d - ctu_cols + 2) / 2, hi = d / 2;                       // the rows cy with 0 <= d - 2 cy < ctu_cols
        if (lo < 0) lo = 0;
        if (hi > ctu_rows - 1) hi = ctu_rows - 1;
        const int cnt = hi >= lo ? hi - lo + 1 : 0;
        if (t < cnt) return (lo + t) * ctu_cols + d - 2 * (lo + t);
        t -= cnt;
    }
}

}  // namespace ks265
