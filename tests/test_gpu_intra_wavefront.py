"""The key picture's CU-granular intra wavefront (intra_recon_kernel<false>: worker work-groups taking CTUs from a ticket, z-count waits per CU) against the
oracle at three picture sizes - partial right / bottom CTUs included - and once while another stream keeps the whole GPU busy with long kernels, so that
only some of the workers are resident at first: the wavefront must still make progress and stay bit-exact."""
from __future__ import annotations

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ks():
    from ks265codec_amd.lib import KsContext
    c = KsContext(0)
    yield c
    c.close()


def _cmp_plane(name, got, exp, stride, org, w, h):
    oy, ox = divmod(org, stride)
    a = got.reshape(-1, stride)[oy:oy + h, ox:ox + w]
    b = exp.reshape(-1, stride)[oy:oy + h, ox:ox + w]
    bad = np.argwhere(a != b)
    assert len(bad) == 0, f"{name}: {len(bad)} mismatches, first at (y,x)={tuple(bad[0])}"


def _key_picture(ks, W, H, qp, seed, busy=None):
    from ks265codec_amd.lib import CU8, KsFrame
    from ks265codec_amd.synth import lambda_q4, make_clip
    from oracle_lib import OraclePipeline

    clip = make_clip(W, H, 1, seed=seed)
    o = OraclePipeline(W, H, qp, lambda_q4(qp), intra=True)
    o.encode(clip[0], "I")
    with KsFrame(ks, W, H, qp, lambda_q4(qp)) as f:
        g = f.geom
        org_y, org_c = g.pad_y * g.stride_y + g.pad_y, g.pad_c * g.stride_c + g.pad_c
        src, rec = f.new_pic(), f.new_pic()
        cu8 = ks.zeros(g.bytes_cu8)
        lvl = [ks.zeros(W * H * 2), ks.zeros(W * H // 2), ks.zeros(W * H // 2)]
        f.load_i420(ks.dev(clip[0]), src)
        f.intra_decide(src, cu8)
        ks.sync()
        if busy is not None:
            busy()                                               # long kernels queued on another stream first
        f.intra_reconstruct(src, cu8, lvl, rec)
        ks.sync()
        assert (ks.host(cu8, CU8) == o.cu8).all(), "cbf differs"
        for k, (a, b, n) in enumerate(zip(lvl, o.lvl, (W * H, W * H // 4, W * H // 4))):
            assert (ks.host(a, np.int16)[:n] == b).all(), f"intra levels differ (component {k})"
        _cmp_plane("rec.y", ks.host(rec.y, np.uint8), o.rec_pre[0], g.stride_y, org_y, W, H)
        _cmp_plane("rec.u", ks.host(rec.u, np.uint8), o.rec_pre[1], g.stride_c, org_c, W // 2, H // 2)
        _cmp_plane("rec.v", ks.host(rec.v, np.uint8), o.rec_pre[2], g.stride_c, org_c, W // 2, H // 2)


@pytest.mark.parametrize("W,H,qp,seed", [(416, 240, 32, 5), (1280, 720, 27, 17), (3840, 2160, 27, 29)])
def test_key_picture_wavefront(ks, W, H, qp, seed):
    _key_picture(ks, W, H, qp, seed)


def test_key_picture_wavefront_under_load(ks):
    torch = ks.torch
    side = torch.cuda.Stream(device=ks.device)
    a = torch.randn(4096, 4096, device=ks.device)
    b = torch.randn(4096, 4096, device=ks.device)
    torch.cuda.synchronize(ks.device)

    def busy():
        with torch.cuda.stream(side):
            c = a
            for _ in range(24):                                  # tens of ms of full-GPU matrix products on the side stream
                c = torch.mm(c, b) * 1e-3

    _key_picture(ks, 1280, 720, 30, 41, busy)
    torch.cuda.synchronize(ks.device)
