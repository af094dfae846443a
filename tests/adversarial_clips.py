"""Adversarial picture content for the parity tests (plain helper, shared by tests/test_adversarial_content_cpu.py, tests/test_gpu_adversarial.py, tests/stream_cases.py
and the golden generator): full-scale differences, flat blocks, saturated neighbours, checkerboards and incompressible noise - what synth.make_clip never produces and
what the range arguments of the kernels (biased 16-bit Hadamard sums, 16-bit interpolation intermediates, level clips, SAO clamps, 16-bit lookahead costs) rest on.
Deterministic (seeded numpy); same layout as synth.make_clip: uint8 [frames, W*H*3/2], planar I420."""
from __future__ import annotations

import numpy as np

FAMILIES = ("flat_flip", "cb1_flip", "cb8_shift", "noise", "bnoise_pan", "edge_ramp")


def _checker(h: int, w: int, period: int, phase: int = 0, dx: int = 0, dy: int = 0) -> np.ndarray:
    yy, xx = np.mgrid[0:h, 0:w]
    return (((((xx - dx) // period) + ((yy - dy) // period) + phase) & 1) * 255).astype(np.uint8)


def make_adversarial(kind: str, W: int, H: int, frames: int, seed: int = 0) -> np.ndarray:
    """flat_flip:  luma 0, 255, 0, ...; both chroma planes in the opposite phase
    cb1_flip:   1-pixel 0/255 checkerboard whose phase advances by one per picture (every sample differs by exactly 255 from the co-located sample of the picture
                before); chroma likewise, U and V in opposite phase
    cb8_shift:  8-pixel checkerboard moving 3 px per picture horizontally; 4-pixel chroma checkerboard moving 1 px per picture vertically (V inverted)
    noise:      uniform 0..255 in all planes, independent per picture
    bnoise_pan: ONE binary 0/255 noise field panned by (2, 1) px per picture (chroma: its own binary field panned (1, 0)): a true motion at full contrast
    edge_ramp:  left part 0, right part 255, one ramp column (128) between them moving 1 px per picture; U constant 0, V constant 255"""
    if kind not in FAMILIES:
        raise ValueError(f"unknown family {kind!r}")
    if W < 2 or H < 2 or W % 2 or H % 2 or frames < 1:
        raise ValueError("even picture sizes and at least one picture")
    rng = np.random.default_rng([seed, FAMILIES.index(kind), W, H])
    w2, h2 = W // 2, H // 2
    if kind == "bnoise_pan":
        fy = (rng.integers(0, 2, (H + frames, W + 2 * frames)) * 255).astype(np.uint8)
        fu = (rng.integers(0, 2, (h2, w2 + frames)) * 255).astype(np.uint8)
        fv = (rng.integers(0, 2, (h2, w2 + frames)) * 255).astype(np.uint8)
    out = np.empty((frames, W * H * 3 // 2), np.uint8)
    for t in range(frames):
        if kind == "flat_flip":
            y = np.full((H, W), 255 * (t & 1), np.uint8)
            u = np.full((h2, w2), 255 * ((t + 1) & 1), np.uint8)
            v = u
        elif kind == "cb1_flip":
            y, u, v = _checker(H, W, 1, t), _checker(h2, w2, 1, t), _checker(h2, w2, 1, t + 1)
        elif kind == "cb8_shift":
            y, u = _checker(H, W, 8, 0, dx=3 * t), _checker(h2, w2, 4, 0, dy=t)
            v = 255 - u
        elif kind == "noise":
            y, u, v = (rng.integers(0, 256, s, dtype=np.uint8) for s in ((H, W), (h2, w2), (h2, w2)))
        elif kind == "bnoise_pan":
            y, u, v = fy[t:t + H, 2 * t:2 * t + W], fu[:, t:t + w2], fv[:, t:t + w2]
        else:
            x0 = (W // 2 + t) % W
            y = np.zeros((H, W), np.uint8)
            y[:, x0] = 128
            y[:, x0 + 1:] = 255
            u, v = np.zeros((h2, w2), np.uint8), np.full((h2, w2), 255, np.uint8)
        out[t] = np.concatenate([np.ascontiguousarray(p).reshape(-1) for p in (y, u, v)])
    return out


def planes(frame: np.ndarray, W: int, H: int):
    """(Y, U, V) views of one I420 picture"""
    return frame[:W * H].reshape(H, W), frame[W * H:W * H * 5 // 4].reshape(H // 2, W // 2), frame[W * H * 5 // 4:].reshape(H // 2, W // 2)
