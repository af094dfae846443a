"""CPU: tests/sao_merge_ref.py, the specification of ks265_frame_cfg.sao = 3 - its NumPy statistics and apply are pinned on the pipeline oracle (with the neighbours disabled it
IS the oracle's sao = 2), and with the neighbours enabled every kind of outcome occurs at sizes small enough for the GPU tests."""
from __future__ import annotations

import numpy as np
import pytest

import sao_merge_cases as K


@pytest.mark.parametrize("W,H", sorted(K.SIZES))
def test_without_neighbours_it_is_the_oracles_reference_decision(W, H):
    for p in K.ippp(W, H, 3, neighbours=False):
        assert (p["records"].view(np.uint8) == p["own_records"].view(np.uint8)).all(), f"{W}x{H} picture {p['d']}: records differ from OraclePipeline(sao=2)"
        assert (p["recon"] == p["own_recon"]).all(), f"{W}x{H} picture {p['d']}: {int((p['recon'] != p['own_recon']).sum())} samples differ from OraclePipeline(sao=2)"


def test_every_kind_of_outcome_occurs():
    for p in K.ippp(416, 240, 3):
        left, up, own = K.merge_counts(p["records"])
        print(f"picture {p['d']}: merge left {left}, merge up {up}, own parameters {own}")
        assert left >= 1 and up >= 1 and own >= 1 and left + up + own == 28


@pytest.mark.parametrize("W,H", sorted(K.SIZES))
def test_a_merged_ctu_holds_its_neighbours_records(W, H):
    cols = (W + 63) // 64
    merged = 0
    for p in K.ippp(W, H, 3):
        r = p["records"].reshape(-1, 3)
        assert (r["rsv"][:, 1:] == 0).all() and set(np.unique(r["rsv"][:, 0])) <= {0, 1} and (r["rsv"][:, 0].sum(axis=1) <= 1).all()
        assert set(np.unique(r["type"])) <= {-1, 0, 1, 2}
        for ctu in range(len(r)):
            ml, mu = r[ctu, 0]["rsv"]
            if not (ml or mu):
                continue
            assert (ctu % cols > 0) if ml else (ctu >= cols)
            n = r[ctu - 1] if ml else r[ctu - cols]
            for f in ("type", "band", "offset"):
                assert (r[ctu][f] == n[f]).all(), f"picture {p['d']} CTU {ctu}: {f} differs from the {'left' if ml else 'upper'} CTU's"
            merged += 1
    assert merged > 0
