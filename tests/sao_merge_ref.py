"""The specification of ks265_frame_cfg.sao = 3 (TEST INFRASTRUCTURE): the reference's SAO decision with its left / up merge candidates, from source and deblocked planes.

  statistics  NumPy, the rules of the pipeline oracle's sao_collect: s8 truncation of org - rec, edge neighbours outside the picture are not counted, category e < 2 ? e : e - 1;
              whole-CTU statistics, in the 312-word layout of ks265o_sao_mode_decision (counts: bands Y / U / V at 0 / 32 / 64, edge classes at 96 + 20 component + 5 class;
              the sums 156 words on);
  chain       the pinned ks265o_sao_mode_decision (tests/golden/sao_decision.npz), CTU by CTU in raster order, with the FINAL records of the left and the upper CTU, masks 0x13;
  records     SAO_PARAM, rsv[0] / rsv[1] of a CTU's luma record = merge left / merge up; a merged CTU's three records are copies of the neighbour's;
  apply       NumPy, the rules of sao_apply_ctu, out of place from the deblocked planes.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

import oracle_lib
from oracle_lib import SAO_PARAM

LAMBDA_SAO_Q8 = (9, 12, 15, 19, 24, 31, 39, 50, 63, 79, 100, 127, 161, 203, 257, 325, 411, 519, 656, 829, 1048, 1324, 1674, 2115, 2673, 3377, 4268, 5393, 6815, 8612, 10883,
                 13752, 17378, 21960, 27750, 35066, 44311, 55994, 70757, 89411, 112984, 142772, 180413, 227978, 288084, 364036, 460012, 581291, 734546, 928205, 1172921, 1482155)
EO_DX, EO_DY = (1, 0, 1, -1), (0, 1, 1, 1)
STATS_WORDS = 312


def chroma_qp(qp: int) -> int:
    return qp if qp < 30 else qp - 6 if qp >= 44 else (29, 30, 31, 32, 33, 33, 34, 34, 35, 35, 36, 36, 37, 37)[qp - 30]


def edge_index(rec: np.ndarray, cls: int) -> np.ndarray:
    """per sample of a plane: 2 + sign(c - a) + sign(c - b) for the two neighbours of edge class cls, 2 (= no category) where one of them lies outside the picture"""
    h, w = rec.shape
    c = rec.astype(np.int32)
    p = np.pad(c, 1)
    dx, dy = EO_DX[cls], EO_DY[cls]
    a = p[1 - dy:1 - dy + h, 1 - dx:1 - dx + w]
    b = p[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
    e = 2 + np.sign(c - a) + np.sign(c - b)
    ys, xs = np.mgrid[0:h, 0:w]
    inside = (xs - dx >= 0) & (xs - dx < w) & (xs + dx >= 0) & (xs + dx < w) & (ys - dy >= 0) & (ys + dy < h)
    return np.where(inside, e, 2)


def picture_stats(src: "list[np.ndarray]", deb: "list[np.ndarray]") -> np.ndarray:
    """src / deb: the planes Y, U, V as 2-D uint8 arrays -> (CTUs, 312) int32 in raster order"""
    H, W = deb[0].shape
    cols, rows = (W + 63) // 64, (H + 63) // 64
    out = np.zeros((rows * cols, STATS_WORDS), np.int32)
    for comp in range(3):
        rec, org, n = deb[comp], src[comp], 64 if comp == 0 else 32
        diff = (org.astype(np.int32) - rec.astype(np.int32)).astype(np.uint8).view(np.int8).astype(np.int64)      # the reference's s8 truncation
        eidx = [edge_index(rec, cls) for cls in range(2)]
        for cy in range(rows):
            for cx in range(cols):
                sl = (slice(cy * n, min((cy + 1) * n, rec.shape[0])), slice(cx * n, min((cx + 1) * n, rec.shape[1])))
                st, c, d = out[cy * cols + cx], rec[sl].ravel(), diff[sl].ravel()
                st[32 * comp:32 * comp + 32] = np.bincount(c >> 3, minlength=32)
                st[156 + 32 * comp:156 + 32 * comp + 32] = np.bincount(c >> 3, weights=d, minlength=32).astype(np.int64)
                for cls in range(2):
                    e = eidx[cls][sl].ravel()
                    use = e != 2
                    cat = np.where(e < 2, e, e - 1)[use]
                    at = 96 + 20 * comp + 5 * cls
                    st[at:at + 4] = np.bincount(cat, minlength=4)
                    st[156 + at:156 + at + 4] = np.bincount(cat, weights=d[use], minlength=4).astype(np.int64)
    return out


def decide(stats: np.ndarray, cols: int, rows: int, qp, neighbours: bool = True) -> np.ndarray:
    """the chain in raster order; qp: one value or one per CTU.  Returns (CTUs * 3) SAO_PARAM records, rsv of the luma record = (merge left, merge up)"""
    o = oracle_lib.lib()
    qps = np.broadcast_to(np.asarray(qp, np.int64).ravel(), (rows * cols,)) if np.ndim(qp) == 0 else np.asarray(qp, np.int64).ravel()
    raw = np.zeros((rows * cols, 32), np.int8)                     # the reference's own 32-byte records: what a neighbour is priced from
    out = np.zeros(rows * cols * 3, SAO_PARAM)
    for ctu in range(rows * cols):
        cx, cy = ctu % cols, ctu // cols
        la, ua = int(neighbours and cx > 0), int(neighbours and cy > 0)
        st = np.ascontiguousarray(stats[ctu], np.int32)
        q = int(qps[ctu])
        o.ks265o_sao_mode_decision(st.ctypes.data_as(C.c_void_p), LAMBDA_SAO_Q8[q], LAMBDA_SAO_Q8[chroma_qp(q)], la, ua,
                                   raw[ctu - 1].ctypes.data_as(C.c_void_p) if la else None, raw[ctu - cols].ctypes.data_as(C.c_void_p) if ua else None,
                                   0x13, 0x13, raw[ctu].ctypes.data_as(C.c_void_p), None)
        r = raw[ctu]
        for comp in range(3):
            t, p = int(r[1 if comp else 0]), out[ctu * 3 + comp]
            p["type"] = -1 if t == -1 else 0 if t == 4 else 1 + t             # this build's codes: -1 off, 0 band offset, 1 + edge class
            if t != -1:
                p["band"] = r[2 if comp == 0 else 2 + comp] if t == 4 else 0
                p["offset"] = r[(5, 0xa, 0xf)[comp]:(5, 0xa, 0xf)[comp] + 4]
        out[ctu * 3]["rsv"] = (r[0x14], r[0x15])
    return out


def apply(deb: "list[np.ndarray]", records: np.ndarray) -> "list[np.ndarray]":
    H, W = deb[0].shape
    cols, rows = (W + 63) // 64, (H + 63) // 64
    res = []
    for comp in range(3):
        rec, n = deb[comp], 64 if comp == 0 else 32
        dst = rec.copy()
        eidx = {}
        for cy in range(rows):
            for cx in range(cols):
                p = records[(cy * cols + cx) * 3 + comp]
                t = int(p["type"])
                if t < 0:
                    continue
                sl = (slice(cy * n, min((cy + 1) * n, rec.shape[0])), slice(cx * n, min((cx + 1) * n, rec.shape[1])))
                c = rec[sl].astype(np.int32)
                offs = p["offset"].astype(np.int32)
                if t == 0:
                    k = (c >> 3) - int(p["band"])
                    o = np.where((k >= 0) & (k < 4), offs[np.clip(k, 0, 3)], 0)
                else:
                    if t - 1 not in eidx:
                        eidx[t - 1] = edge_index(rec, t - 1)
                    e = eidx[t - 1][sl]
                    o = np.where(e != 2, offs[np.clip(np.where(e < 2, e, e - 1), 0, 3)], 0)
                dst[sl] = np.clip(c + o, 0, 255).astype(np.uint8)
        res.append(dst)
    return res


def sao_merge(src: "list[np.ndarray]", deb: "list[np.ndarray]", qp, neighbours: bool = True):
    """-> (records, the applied planes)"""
    H, W = deb[0].shape
    records = decide(picture_stats(src, deb), (W + 63) // 64, (H + 63) // 64, qp, neighbours)
    return records, apply(deb, records)


# ---- padded pictures (oracle_lib.HostPic / the device's planes as host arrays)
def planes_of(pic, geom, W: int, H: int) -> "list[np.ndarray]":
    """the picture area of a padded picture's three planes (copies; the buffers are a little longer than rows x stride)"""
    y = pic.y[:geom.rows_y * geom.stride_y].reshape(geom.rows_y, geom.stride_y)[geom.pad_y:geom.pad_y + H, geom.pad_y:geom.pad_y + W]
    u = pic.u[:geom.rows_c * geom.stride_c].reshape(geom.rows_c, geom.stride_c)[geom.pad_c:geom.pad_c + H // 2, geom.pad_c:geom.pad_c + W // 2]
    v = pic.v[:geom.rows_c * geom.stride_c].reshape(geom.rows_c, geom.stride_c)[geom.pad_c:geom.pad_c + H // 2, geom.pad_c:geom.pad_c + W // 2]
    return [y.copy(), u.copy(), v.copy()]


def i420_of(planes: "list[np.ndarray]") -> np.ndarray:
    return np.concatenate([p.ravel() for p in planes])


def sao_merge_pipeline(op, qp, neighbours: bool = True):
    """on an OraclePipeline after encode(): its source and deblocked picture -> (records, padded HostPic of the applied picture, its planes)"""
    W, H = op.cfg.width, op.cfg.height
    records, planes = sao_merge(planes_of(op.src, op.geom, W, H), planes_of(op.rec, op.geom, W, H), qp, neighbours)
    out = oracle_lib.HostPic(op.geom)
    op.load(out, i420_of(planes))                        # kso_load_i420 pads the borders the way kso_pad_picture does
    return records, out, planes
