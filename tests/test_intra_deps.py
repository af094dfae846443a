"""The intra wavefront's dependency rule (ks265codec_amd/csrc/intra_deps.h, host-callable) against H.265 6.4.1 availability, exhaustively: every CU position
and size (8 / 16 / 32) of CTUs in the first row and column, interior ones and partial right / bottom CTUs.  For every CU:
  * every neighbour sample it may read that is available and lies in another CTU is covered by a waited z-count;
  * no waited CTU has a raster index at or above the CU's own;
  * no wait asks for a block that is not available to the CU.
And the key pictures' ticket order (ks_ctu_of_ticket) is a permutation of the CTUs in which every CTU a CU waits for comes earlier."""
from __future__ import annotations

import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include "intra_deps.h"
using namespace ks265;
int main(int argc, char **argv)
{
    const int W = atoi(argv[1]), H = atoi(argv[2]), cols = (W + 63) / 64, rows = (H + 63) / 64;
    if (argc == 3) {                                           // the ticket order
        for (int t = 0; t < cols * rows; ++t) printf("%d\n", ks_ctu_of_ticket(t, cols, rows));
        return 0;
    }
    for (int i = 3; i + 1 < argc; i += 2) {
        const int cx = atoi(argv[i]), cy = atoi(argv[i + 1]);
        for (int n8 = 1; n8 <= 4; n8 *= 2)
            for (int ly = 0; ly < 8; ly += n8)
                for (int lx = 0; lx < 8; lx += n8)
                    for (int which = 0; which < KS_NBR_COUNT; ++which) {
                        int ctu;
                        const int need = ks_intra_need(which, cols, W / 8, H / 8, cx, cy, lx, ly, n8, &ctu);
                        if (need) printf("%d %d %d %d %d %d %d %d\n", cx, cy, lx, ly, n8, which, ctu, need);
                    }
    }
    return 0;
}
"""


def zorder(bx, by):
    z = 0
    for b in range(3):
        z |= ((bx >> b) & 1) << (2 * b) | ((by >> b) & 1) << (2 * b + 1)
    return z


def available(W, H, x, y, nx, ny):
    """H.265 6.4.1 with 64x64 CTUs and 4x4 minimum blocks: is sample (nx, ny) available to the block whose first sample is (x, y)?"""
    if nx < 0 or ny < 0 or nx >= W or ny >= H:
        return False
    cols = (W + 63) // 64
    ca, na = (y // 64) * cols + x // 64, (ny // 64) * cols + nx // 64
    if na != ca:
        return na < ca

    def z4(px, py):                                            # z-scan order of the 4x4 block inside the CTU
        bx, by, z = (px % 64) // 4, (py % 64) // 4, 0
        for b in range(4):
            z |= ((bx >> b) & 1) << (2 * b) | ((by >> b) & 1) << (2 * b + 1)
        return z
    return z4(nx, ny) < z4(x, y)


def ctus_to_check(W, H):
    cols, rows = (W + 63) // 64, (H + 63) // 64
    if cols * rows <= 300:
        return [(cx, cy) for cy in range(rows) for cx in range(cols)]
    xs = sorted({0, 1, 2, cols // 2, cols - 2, cols - 1})
    ys = sorted({0, 1, 2, rows // 2, rows - 2, rows - 1})
    return [(cx, cy) for cy in ys for cx in xs]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("intra_deps")
    src, exe = d / "drv.cpp", d / "drv"
    src.write_text(DRIVER)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "ks265codec_amd", "csrc"), str(src), "-o", str(exe)])
    return str(exe)


@pytest.mark.parametrize("W,H", [(416, 240), (1280, 720), (3840, 2160), (200, 136)])
def test_intra_dependency_rule(driver, W, H):
    cols = (W + 63) // 64
    ctus = ctus_to_check(W, H)
    out = subprocess.run([driver, str(W), str(H)] + [str(v) for c in ctus for v in c], capture_output=True, text=True, check=True).stdout
    waits = {}
    for line in out.splitlines():
        cx, cy, lx, ly, n8, which, ctu, need = map(int, line.split())
        waits.setdefault((cx, cy, lx, ly, n8), []).append((which, ctu, need))
    ncu = 0
    for cx, cy in ctus:
        own = cy * cols + cx
        for n8 in (1, 2, 4):
            n = 8 * n8
            for ly in range(0, 8, n8):
                for lx in range(0, 8, n8):
                    x0, y0 = cx * 64 + lx * 8, cy * 64 + ly * 8
                    if x0 + n > W or y0 + n > H:
                        continue                                     # no CU reaches outside the picture
                    ncu += 1
                    got = waits.get((cx, cy, lx, ly, n8), [])
                    assert len({w for w, _, _ in got}) == len(got)
                    need = {}
                    for which, ctu, z in got:
                        # no wait on a CTU at or after this one, none beyond a whole CTU, none for a block the CU may not read
                        assert 0 <= ctu < own, (W, H, cx, cy, lx, ly, n8, which, ctu)
                        assert 1 <= z <= 64
                        bx = next(b for b in range(64) if zorder(b % 8, b // 8) == z - 1)
                        kx, ky = (ctu % cols) * 64 + (bx % 8) * 8, (ctu // cols) * 64 + (bx // 8) * 8
                        assert available(W, H, x0, y0, kx, ky), (W, H, cx, cy, lx, ly, n8, which, ctu, z)
                        need[ctu] = max(need.get(ctu, 0), z)
                    # every neighbour sample (H.265 8.4.4.2.2: 2n left incl. below-left, the corner, 2n above incl. above-right) that is available and lies in
                    # another CTU is covered
                    samples = [(x0 - 1, y0 + k) for k in range(-1, 2 * n)] + [(x0 + k, y0 - 1) for k in range(2 * n)]
                    for sx, sy in samples:
                        if not available(W, H, x0, y0, sx, sy):
                            continue
                        k = (sy // 64) * cols + sx // 64
                        if k == own:
                            continue
                        z = zorder((sx % 64) // 8, (sy % 64) // 8)
                        assert need.get(k, 0) > z, (W, H, cx, cy, lx, ly, n8, (sx, sy), k, z, got)
    assert ncu > 0


@pytest.mark.parametrize("W,H", [(416, 240), (1280, 720), (3840, 2160), (200, 136), (64, 64), (64, 1024), (1024, 64)])
def test_ticket_order(driver, W, H):
    cols, rows = (W + 63) // 64, (H + 63) // 64
    order = [int(v) for v in subprocess.run([driver, str(W), str(H)], capture_output=True, text=True, check=True).stdout.split()]
    assert sorted(order) == list(range(cols * rows))
    ticket = {k: t for t, k in enumerate(order)}
    ctus = [(cx, cy) for cy in range(rows) for cx in range(cols)]
    out = subprocess.run([driver, str(W), str(H)] + [str(v) for c in ctus for v in c], capture_output=True, text=True, check=True).stdout
    for line in out.splitlines():
        cx, cy, lx, ly, n8, which, ctu, need = map(int, line.split())
        assert ticket[ctu] < ticket[cy * cols + cx], (W, H, cx, cy, which, ctu)
