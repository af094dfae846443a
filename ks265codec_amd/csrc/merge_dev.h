// merge_dev.h — the spatial merge candidates of H.265 8.5.3.2.3 on a CU map, once: the merge pass (frame_me.hip) picks among them, the skip pass (frame_skip.hip) tries them without
// residual, and the writer's merge index counts them the same way - a CU's candidate k must be the same motion everywhere.  Device only.
#pragma once
#include "frame_common.h"

// the 8x8 tiles of a CTU in z-order: tile z lies at (ks_z_x(z), ks_z_y(z)), in tiles; ks_z_of_8 = the z-scan address of the tile that holds sample (x, y)
__device__ __forceinline__ int ks_z_x(int z) { return (z & 1) | ((z >> 1) & 2) | ((z >> 2) & 4); }
__device__ __forceinline__ int ks_z_y(int z) { return ((z >> 1) & 1) | ((z >> 2) & 2) | ((z >> 3) & 4); }
__device__ __forceinline__ int ks_z_of_8(int x, int y)
{
    const int bx = (x >> 3) & 7, by = (y >> 3) & 7;
    return (bx & 1) | ((by & 1) << 1) | ((bx & 2) << 1) | ((by & 2) << 2) | ((bx & 4) << 2) | ((by & 4) << 3);
}

// a candidate's motion as its CU record holds it: dir = inter_dir (MR: direction | idx0 << 4 | idx1 << 6, else the direction alone); the vectors of a list the motion does not
// use are whatever the record holds
struct KsMotion { int dir, mvx, mvy, mv1x, mv1y; bool ok; };

// candidate k of the node (x, y, n) from the map: A1 B1 B0 A0 B2 (inside the picture, earlier in z-scan order, inter), 5 = the zero vector (bi_zero: of both lists).
// MR: the neighbour's pictures come with its motion
template <bool MR>
__device__ __forceinline__ KsMotion ks_merge_cand(const KsGeom &g, const ks265_cu8 *map, int x, int y, int n, int k, bool bi_zero)
{
    KsMotion m; m.dir = bi_zero ? 3 : 1; m.mvx = m.mvy = m.mv1x = m.mv1y = 0; m.ok = true;
    if (k == 5) return m;
    const int nx = k == 1 ? x + n - 1 : k == 2 ? x + n : x - 1, ny = k == 0 ? y + n - 1 : k == 3 ? y + n : y - 1;       // A1 B1 B0 A0 B2
    m.ok = false;
    if (nx < 0 || ny < 0 || nx >= g.W || ny >= g.H) return m;
    const int ctb = (y >> 6) * g.ctu_cols + (x >> 6), nctb = (ny >> 6) * g.ctu_cols + (nx >> 6);
    if (nctb > ctb || (nctb == ctb && ks_z_of_8(nx, ny) >= ks_z_of_8(x, y))) return m;
    const ks265_cu8 c = map[(long)(ny >> 3) * g.w8 + (nx >> 3)];
    if (c.pred_mode != 0 || (c.log2_cu & 15) < 3) return m;
    m.dir = MR ? (int)c.inter_dir : (c.inter_dir & 3); m.mvx = c.mvx; m.mvy = c.mvy; m.mv1x = c.mv1x; m.mv1y = c.mv1y; m.ok = true;
    // a neighbour's vector may come from a CTU with another window offset: taken over here it must keep this CU's block inside the planes' margin
    if ((m.dir & 1) && (x + (m.mvx >> 2) < -70 || x + (m.mvx >> 2) + n > g.W + 70 || y + (m.mvy >> 2) < -70 || y + (m.mvy >> 2) + n > g.H + 70)) m.ok = false;
    if ((m.dir & 2) && (x + (m.mv1x >> 2) < -70 || x + (m.mv1x >> 2) + n > g.W + 70 || y + (m.mv1y >> 2) < -70 || y + (m.mv1y >> 2) + n > g.H + 70)) m.ok = false;
    return m;
}

// the same motion: equal dir, equal vectors of the lists dir uses (equal dir: both use the same lists, so zeroing the unused vectors first changes nothing)
__device__ __forceinline__ bool ks_motion_same(const KsMotion &a, const KsMotion &b)
{
    return a.dir == b.dir && (!(a.dir & 1) || (a.mvx == b.mvx && a.mvy == b.mvy)) && (!(a.dir & 2) || (a.mv1x == b.mv1x && a.mv1y == b.mv1y));
}
