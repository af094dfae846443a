"""The one place that knows how the CPU tests of the encoder host are made: how the host sources and a stand-in of the device library (tests/hip_stub*.c) are compiled,
loaded and opened, how a session is driven to its stream, and the ctypes mirrors of the API structs (include/ks265_enc.h).  A plain module: importing it builds nothing,
writes nothing and reads nothing but tests/golden/qy265_layout.json.

  * build_host_lib / build_host_program compile a given (sources, defines, sanitize) once per process.  A program is shared as it is; a LIBRARY is loaded through
    load_host_lib, which copies it to a path of its own first: every module that loads one has a private instance with its own static state - the call log's path (read
    once), the numbering of contexts, frames and events from the first call on, the process defaults of ks265_enc_set_default.  dlopen of one path would share all that.
  * sanitized code is a stand-alone program run as a child process, the sanitizers' runtimes linked into it; nothing sanitized is ever loaded into Python.
  * drive() is the session every stream test runs: feed, collect, flush, close, and nothing of the stand-in's left alive."""
from __future__ import annotations

import atexit
import ctypes as C
import hashlib
import itertools
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

import picture_window_ref as pw

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOST = os.path.join(ROOT, "ks265codec_amd", "host")
LAY = json.load(open(os.path.join(HERE, "golden", "qy265_layout.json")))
QY_OK, QY_FAIL, QY_POINTER, QY_NOTSUPPORTED = 0, -0x7FFFFFFF, -0x7FFFFFFD, -0x7FFFFFFC
IN_I420, IN_NV12, IN_RGB = 0, 1, 2
LOG_CB = C.CFUNCTYPE(None, C.c_char_p)


class YUV(C.Structure):
    _fields_ = [("iWidth", C.c_int), ("iHeight", C.c_int), ("pData", C.POINTER(C.c_ubyte) * 3), ("iStride", C.c_int * 3)]


class Picture(C.Structure):
    _fields_ = [("iSliceType", C.c_int), ("poc", C.c_int), ("pts", C.c_longlong), ("dts", C.c_longlong), ("yuv", C.POINTER(YUV))]


class Nal(C.Structure):
    _fields_ = [("naltype", C.c_int), ("tid", C.c_int), ("iSize", C.c_int), ("pts", C.c_longlong), ("pPayload", C.POINTER(C.c_ubyte))]


class DevPicture(C.Structure):
    _fields_ = [("format", C.c_int), ("device", C.c_int), ("plane", C.c_void_p * 3), ("pitch", C.c_int * 3), ("pixel_step", C.c_int),
                ("matrix", C.c_int), ("full_range", C.c_int), ("stream", C.c_void_p), ("pts", C.c_longlong)]


class Roi(C.Structure):
    _fields_ = [("type", C.c_int), ("log2_block", C.c_int), ("device", C.c_int), ("data", C.c_void_p), ("pitch", C.c_int), ("stream", C.c_void_p)]


# ------------------------------------------------------------------ building

WARN = ["-std=gnu11", "-Wall", "-Wextra", "-Werror"]
# (the sanitizers' runtimes inside the program: it starts whatever else the environment preloads into every process)
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-static-libasan", "-static-libubsan"]
_built: dict[tuple, str] = {}
_scratch_dir = None
_serial = itertools.count()


def cc(*args) -> None:
    """the compiler, for everything under tests/"""
    subprocess.check_call(["gcc", *[str(a) for a in args]])


def _scratch() -> str:
    """the process's directory for what is built and loaded, removed at exit"""
    global _scratch_dir
    if _scratch_dir is None:
        _scratch_dir = tempfile.mkdtemp(prefix="ks265_host_")
        atexit.register(shutil.rmtree, _scratch_dir, ignore_errors=True)
    return _scratch_dir


def _src(name: str) -> str:
    return name if os.path.isabs(name) else os.path.join(HERE, name)


def _build(name, flags, sources, stub, defines, extra_sources, host_dir) -> str:
    host_dir = host_dir or HOST
    sources = [*sources, *[_src(s) for s in extra_sources]]
    tail = ["-lpthread", "-lm"]
    if stub:                                                            # the two host sources and the stand-in, against the oracle
        sources += [os.path.join(host_dir, "ks265_enc.c"), os.path.join(host_dir, "ks265_stream.c"), _src(stub)]
        tail = ["-L", os.path.join(ROOT, "oracle"), "-lks265_oracle", "-Wl,-rpath," + os.path.join(ROOT, "oracle")] + tail
    key = (name, tuple(flags), tuple(sources), tuple(defines))
    if key not in _built:
        if stub:
            from oracle_lib import build_oracle
            build_oracle()
        d = os.path.join(_scratch(), "b%d" % next(_serial))
        os.mkdir(d)
        out = os.path.join(d, name)
        cc(*flags, *WARN, *["-D" + x for x in defines], "-I", os.path.join(ROOT, "include"), "-I", host_dir, "-o", out, *sources, *tail)
        _built[key] = out
    return _built[key]


def build_host_lib(stub: str, defines=(), extra_sources=(), host_dir: str | None = None) -> str:
    """the path of a shared library of the host (of this tree, or the sources in `host_dir`) and tests/<stub>.  For a child process as it is; into this process through
    load_host_lib"""
    return _build("libks265enc_stub.so", ["-O2", "-fPIC", "-shared"], [], stub, defines, extra_sources, host_dir)


def build_host_program(main_c: str, stub: str | None = None, sanitize: bool = True, defines=(), extra_sources=(), host_dir: str | None = None) -> str:
    """the path of a program made of tests/<main_c> (or an absolute path) - with `stub` also of the host and that stand-in - under the sanitizers or plain"""
    name = os.path.splitext(os.path.basename(main_c))[0] + ("_asan" if sanitize else "")
    return _build(name, ["-O1", *SANITIZE] if sanitize else ["-O2"], [_src(main_c)], stub, defines, extra_sources, host_dir)


def build_host_cli(stub: str = "hip_stub.c", defines=(), host_dir: str | None = None) -> str:
    """the encoder's command line (ks265_cli.c of the host) on a stand-in"""
    return build_host_program(os.path.join(host_dir or HOST, "ks265_cli.c"), stub=stub, sanitize=False, defines=defines, host_dir=host_dir)


def load_host_lib(path: str, call_log: str | None = None, mode: int = C.DEFAULT_MODE):
    """a private instance of the library: a fresh copy under a new path, the restypes every module needs.  call_log: the stand-in writes its call log there (it reads
    KS265_STUB_CALL_LOG once, at the library's first logged call - an open and close made here); the path is kept as lib.call_log_path"""
    mine = os.path.join(_scratch(), "l%d_%s" % (next(_serial), os.path.basename(path)))
    shutil.copy(path, mine)
    lib = C.CDLL(mine, mode=mode)
    lib.QY265EncoderOpen.restype = C.c_void_p
    if hasattr(lib, "ks265_stub_live"):
        lib.ks265_stub_live.restype = C.c_long
    if call_log is not None:
        old = os.environ.get("KS265_STUB_CALL_LOG")
        os.environ["KS265_STUB_CALL_LOG"] = call_log
        try:
            lib.QY265EncoderClose(open_handle(lib, 128, 72, lanes=1))   # (the first logged call)
        finally:
            os.environ.pop("KS265_STUB_CALL_LOG", None)
            if old is not None:
                os.environ["KS265_STUB_CALL_LOG"] = old
        lib.call_log_path = call_log
    return lib


# ------------------------------------------------------------------ handles

def fresh_config(lib, w, h, params=(), latency=b"default"):
    """QY265ConfigDefaultPreset("medium") and the parameters every host test starts from, then `params`"""
    cfg = (C.c_uint8 * LAY["sizeof_config"])()
    assert lib.QY265ConfigDefaultPreset(cfg, b"medium", None, latency) == 0
    for k, v in (("wdt", w), ("hgt", h), ("fr", 50), ("rc", 0), ("qp", 34), ("threads", 4), ("log", 1), *params):
        assert lib.QY265ConfigParse(cfg, k.encode(), str(v).encode()) == 0, k
    return cfg


def try_open(lib, w, h, params=(), lanes=None, latency=b"default", env=None, roi=False, defaults=()):
    """(handle, error code) of QY265EncoderOpen.  lanes: KS265_GOP_LANES for the open (None: as the environment has it); env: more variables for the open; roi / defaults:
    process defaults (ks265_enc_set_default; names, or a dict of their values) switched on for this open alone.  Every variable is restored"""
    env = {k: str(v) for k, v in (env or {}).items()}
    if lanes is not None:
        env["KS265_GOP_LANES"] = str(lanes)
    defaults = dict(defaults if isinstance(defaults, dict) else dict.fromkeys(defaults, 1), **({"roi": 1} if roi else {}))
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        cfg = fresh_config(lib, w, h, params, latency)
        for name, v in defaults.items():
            assert lib.ks265_enc_set_default(name.encode(), C.c_int(v)) == 0
        err = C.c_int(0)
        hd = C.c_void_p(lib.QY265EncoderOpen(cfg, C.byref(err)))
        for name in defaults:
            assert lib.ks265_enc_set_default(name.encode(), C.c_int(0)) == 0      # read at open: the handle keeps it
        return hd, err.value
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def open_handle(lib, w, h, **kw):
    hd, err = try_open(lib, w, h, **kw)
    assert hd.value, hex(err & 0xFFFFFFFF)
    return hd


# ------------------------------------------------------------------ sessions

def nal_bytes(nal, nn) -> bytes:
    return b"".join(C.string_at(nal[i].pPayload, nal[i].iSize) for i in range(nn.value) if nal[i].iSize > 0)


def drive(lib, hd, submits, after=None) -> bytes:
    """the session: every submit(nal, nn, outp) -> rc of `submits` is one picture and must be QY_OK; the handle is flushed and closed, and nothing of the stand-in's may be
    left alive.  after(): called behind every call that may have handed pictures out.  The stream."""
    nal, nn, outp, bs = C.POINTER(Nal)(), C.c_int(0), Picture(), bytearray()

    def collect():
        bs.extend(nal_bytes(nal, nn))
        if after:
            after()

    for t, submit in enumerate(submits):
        rc = submit(nal, nn, outp)
        assert rc == QY_OK, (t, hex(rc & 0xFFFFFFFF))
        collect()
    while lib.QY265EncoderDelayedFrames(hd) > 0:
        assert lib.QY265EncoderEncodeFrame(hd, C.byref(nal), C.byref(nn), None, C.byref(outp), 0) == QY_OK
        collect()
    lib.QY265EncoderClose(hd)
    assert [lib.ks265_stub_live(k) for k in range(5)] == [0] * 5, "contexts, frame objects, events, device and pinned blocks"
    return bytes(bs)


def packed_yuv(p: np.ndarray, w, h) -> YUV:
    """the QY265YUV of a packed I420 picture where it lies"""
    yuv = YUV()
    yuv.iWidth, yuv.iHeight = w, h
    yuv.iStride[0], yuv.iStride[1], yuv.iStride[2] = w, w // 2, w // 2
    for k, off in enumerate((0, w * h, w * h * 5 // 4)):
        yuv.pData[k] = C.cast(p.ctypes.data + off, C.POINTER(C.c_ubyte))
    return yuv


def rows(q: np.ndarray, extra: int) -> np.ndarray:
    """plane q in a buffer of its own with `extra` bytes of 0xA5 behind every row"""
    b = np.full((q.shape[0], q.shape[1] + extra), 0xA5, np.uint8)
    b[:, :q.shape[1]] = q
    return b


def host_picture(lib, hd, p: np.ndarray, w, h, pts=0, way="p"):
    """a submit for packed I420 picture p through QY265EncoderEncodeFrame.  way p: the packed picture where it lies; c / s: plane by plane in buffers of their own, rows
    contiguous / 9 bytes apart; a: written into an acquired slot (where the handle has none to give: as c)"""
    def submit(nal, nn, outp):
        pic, yuv, keep = Picture(), YUV(), []
        if way == "p":
            yuv = packed_yuv(p, w, h)
        elif way == "a" and lib.ks265_enc_acquire_input(hd, C.byref(yuv)) == QY_OK:
            assert (yuv.iWidth, yuv.iHeight, tuple(yuv.iStride)) == (w, h, (w, w // 2, w // 2))
            for k, q in enumerate(pw.planes(p, w, h)):
                C.memmove(yuv.pData[k], np.ascontiguousarray(q).ctypes.data, q.size)
        else:
            yuv.iWidth, yuv.iHeight = w, h
            for k, q in enumerate(pw.planes(p, w, h)):
                keep.append(rows(q, 9 if way == "s" else 0))
                yuv.pData[k], yuv.iStride[k] = C.cast(keep[k].ctypes.data, C.POINTER(C.c_ubyte)), keep[k].strides[0]
        pic.yuv, pic.pts = C.pointer(yuv), pts
        return lib.QY265EncoderEncodeFrame(hd, C.byref(nal), C.byref(nn), C.byref(pic), C.byref(outp), 0)
    return submit


def dev_pic(bufs, offs, pitches, code, pts=0, step=0, matrix=0, full_range=0) -> DevPicture:
    """the descriptor of a picture in "device" memory: plane k lies offs[k] bytes into bufs[k] (into the only buffer where there is one)"""
    d = DevPicture()
    d.format, d.device, d.stream, d.pts, d.pixel_step, d.matrix, d.full_range = code, 0, None, pts, step, matrix, full_range
    for k, off in enumerate(offs):
        d.plane[k] = bufs[min(k, len(bufs) - 1)].ctypes.data + off
    for k, p in enumerate(pitches):
        d.pitch[k] = p
    return d


def device_picture(lib, hd, bufs, offs, pitches, code, pts=0, step=0, matrix=0, full_range=0, scaled=None):
    """a submit for a copy of the picture dev_pic describes, through ks265_enc_encode_device_frame or (scaled=(sw, sh, filter)) the scaled entry.  The copy is the
    caller's again once the call has returned (the stand-in runs everything inside it): it is written over with 0x5A"""
    def submit(nal, nn, outp):
        own = [np.array(b, order="C") for b in bufs]
        d = dev_pic(own, offs, pitches, code, pts, step, matrix, full_range)
        if scaled:
            rc = lib.ks265_enc_encode_device_frame_scaled(hd, C.byref(nal), C.byref(nn), C.byref(d), scaled[0], scaled[1], scaled[2], C.byref(outp))
        else:
            rc = lib.ks265_enc_encode_device_frame(hd, C.byref(nal), C.byref(nn), C.byref(d), C.byref(outp))
        for b in own:
            b[...] = 0x5A
        return rc
    return submit


def i420_picture(lib, hd, p, w, h, pts=0, nv12=False, extra=0, scaled=None):
    """device_picture for packed I420 picture p as I420 or NV12 planes, rows `extra` bytes apart (extra 0: the packed picture as one block)"""
    if not extra and not nv12:
        return device_picture(lib, hd, [p], (0, w * h, w * h * 5 // 4), (w, w // 2, w // 2), IN_I420, pts, scaled=scaled)
    pl = pw.planes(p, w, h)
    if nv12:
        uv = np.empty((h // 2, w), np.uint8)
        uv[:, 0::2], uv[:, 1::2] = pl[1], pl[2]
        pl = [pl[0], uv]
    bufs = [rows(q, extra) for q in pl]
    return device_picture(lib, hd, bufs, [0] * len(bufs), [b.strides[0] for b in bufs], IN_NV12 if nv12 else IN_I420, pts, scaled=scaled)


def preceded(fn, submit):
    """submit, with fn() called right in front of it"""
    def both(nal, nn, outp):
        fn()
        return submit(nal, nn, outp)
    return both


def session(lib, w, h, pictures, ways="c", lanes=1, latency=b"default", params=(), recon=None):
    """one w x h handle fed packed I420 `pictures`, picture t by way ways[t % len(ways)]: c contiguous, s strided, a an acquired slot, d / n a device I420 / NV12 picture with
    pitches of its own.  recon: the reconstruction is dumped there.  The stream."""
    hd = open_handle(lib, w, h, lanes=lanes, latency=latency, params=params)
    if recon:
        assert lib.ks265_enc_set_recon_file(hd, recon.encode()) == QY_OK
    if set(ways) & set("dn"):
        assert lib.ks265_enc_enable_device_input(hd) == QY_OK
    way = lambda t: ways[t % len(ways)]
    return drive(lib, hd, (i420_picture(lib, hd, p, w, h, t, nv12=way(t) == "n", extra=5) if way(t) in "dn" else host_picture(lib, hd, p, w, h, t, way(t)) for t, p in enumerate(pictures)))


# ------------------------------------------------------------------ what the tests share

def nals(stream: bytes) -> list[tuple[int, bytes]]:
    """(type, bytes) of every NAL unit, start codes dropped"""
    parts = stream.split(b"\x00\x00\x01")[1:]
    return [((p[0] >> 1) & 63, p.rstrip(b"\x00") if i + 1 < len(parts) else p) for i, p in enumerate(parts)]


def calls(lib) -> int:
    """lines of the call log so far"""
    return sum(1 for _ in open(lib.call_log_path))


def logged(lib, fn):
    """(fn's result, the call log's lines it added: `thread name context frame event arg`)"""
    before = calls(lib)
    out = fn()
    return out, [ln for ln in open(lib.call_log_path).read().split("\n")[before:] if ln]


def same_calls(log):
    """the lines without their thread numbers, sorted; contexts, frames and events - numbered by the stand-in from its first call on - counted from the section's first"""
    rows = [ln.split(" ")[1:] for ln in log]
    base = {k: min((int(r[i][1:]) for r in rows if r[i] != "-"), default=0) for i, k in ((1, "c"), (2, "f"), (3, "e"))}
    return sorted(" ".join([r[0]] + [x if x == "-" else "%s%d" % (x[0], int(x[1:]) - base[x[0]]) for x in r[1:4]] + r[4:]) for r in rows)


class EnCall(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("w", "h", "edge_gain", "edge_core", "edge_limit", "edge_over", "color_gain", "has_src", "src_is_hist")]


def en_calls(lib):
    """the enhance calls tests/hip_stub_enhance.c recorded (read by the enhancement's tests and by those of the filter in front of it)"""
    buf = (EnCall * 4096)()
    n = lib.ks265_stub_enhance_calls(buf, 4096)
    return [(c.w, c.h, (c.edge_gain, c.edge_core, c.edge_limit, c.edge_over, c.color_gain), c.has_src, c.src_is_hist) for c in buf[:n]]


def clip(w, h, n, seed):
    """n moving packed I420 pictures"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    out = []
    for t in range(n):
        y = np.clip(128 + 90 * np.sin(0.11 * (xx + 2 * t)) * np.cos(0.07 * (yy + 3 * t)) + rng.integers(0, 6, (h, w)), 0, 255).astype(np.uint8)
        u = np.clip(128 + 50 * np.sin(0.05 * (xx[::2, ::2] + t)), 0, 255).astype(np.uint8)
        v = np.clip(128 + 50 * np.cos(0.09 * (yy[::2, ::2] + t)), 0, 255).astype(np.uint8)
        out.append(pw.pack([y, u, v]))
    return out


def edgy_clip(w, h, n, seed):
    """clip() with a hard-edged box moving over it and saturated chroma corners"""
    out = []
    for t, p in enumerate(clip(w, h, n, seed)):
        y, u, v = [q.copy() for q in pw.planes(p, w, h)]
        y[20 + t:60 + t, 30 + 3 * t:90 + 3 * t] = 200
        y[70:74, :] = 30
        u[:8, :8], v[:8, -8:], u[-8:, -8:], v[-8:, :8] = 0, 255, 255, 3
        out.append(pw.pack([y, u, v]))
    return out


def filter_program(exe, w, h, n, out, latency, *params):
    """one run of tests/input_filter_main.c under the leak checker; per kind of stand-in call (`pad`, `denoise`, `enhance`, `hdr`) the records it printed, each a dict of the
    record's fields"""
    r = subprocess.run([exe, str(w), str(h), str(n), out, latency, *params], capture_output=True, text=True, env={**os.environ, "KS265_GOP_LANES": "1", "ASAN_OPTIONS": "detect_leaks=1"})
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    recs = {"pad": [], "denoise": [], "enhance": [], "hdr": []}
    for ln in r.stdout.splitlines():
        kind, *fields = ln.split()
        if kind in recs:
            recs[kind].append({k: int(v) for k, v in (f.split("=") for f in fields)})
    return recs


def lane_put_env(case: dict, **more) -> dict:
    """the variables of a case of tests/lane_put_main.c; nothing else of KS265_* comes in from outside.  One lane and no lookahead unless the case says otherwise"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("KS265_")}
    env.update({"KS265_GOP_LANES": "1", "KS265_NO_AUTO_LOOKAHEAD": "1"})
    env.update({k: str(v) for k, v in case.get("env", {}).items()})
    env.update(more)
    return {k: v for k, v in env.items() if v != ""}


def cli_encode(stub, out, opts, env=None, size=(200, 136)) -> bytes:
    """one run of the CLI stub["exe"] on the clip stub["yuv"] at constant QP; KS265_GPB reaches it only through `env`"""
    e = {k: v for k, v in os.environ.items() if k not in ("KS265_GPB", "KS265_GOP_LANES")}
    e.update({k: str(v) for k, v in (env or {}).items()})
    r = subprocess.run([stub["exe"], "-i", stub["yuv"], "-wdt", str(size[0]), "-hgt", str(size[1]), "-fr", "50", "-preset", "slow", "-rc", "0", "-qp", "30", "-threads", "3",
                        "-b", str(out), *opts], capture_output=True, text=True, timeout=120, env=e)
    assert r.returncode == 0 and "H265 encoder passed!!!" in r.stdout, r.stdout[-800:] + r.stderr[-800:]
    return open(out, "rb").read()


# the sessions of the pictures handed back out (tests/test_device_recon_host_cpu.py, tests/test_analysis_host_cpu.py): 13 random 128x72 pictures in turn, and the GOP shapes
CLIP = np.random.default_rng(17).integers(0, 256, (13, 128 * 72 * 3 // 2), dtype=np.uint8)
SESSIONS = {
    "ippp": dict(n=40, params=(("iper", 32), ("bframes", 0))),
    "default_gop": dict(n=40, params=(("iper", 32),)),
    "two_lanes": dict(n=100, params=(("iper", 32), ("bframes", 0)), env={"KS265_GOP_LANES": "2"}),
    "zerolatency": dict(n=20, params=(("iper", 32), ("bframes", 0)), latency=b"zerolatency"),
}


def submit_order_cases() -> dict:
    """the cases of tests/golden/submit_order.json (tests/test_submit_order_cpu.py): the scheduler thread's calls, pinned"""
    return json.load(open(os.path.join(HERE, "golden", "submit_order.json")))["cases"]


def scheduler_trace(so: str, case: dict, log: str) -> list[str]:
    """one run of tests/host_driver.py (128x72, one lane); the lines of the thread that issued the ks265_encode_picture* calls, without the thread column"""
    if os.path.exists(log):
        os.remove(log)
    env = dict(os.environ, KS265_STUB_LIB=so, KS265_STUB_CALL_LOG=log, KS265_GOP_LANES="1", **{k: str(v) for k, v in case["env"].items()})
    args = [sys.executable, os.path.join(HERE, "host_driver.py"), ROOT, str(case["n"]), str(case["iper"]), str(case["bframes"]), "128", "72"]
    r = subprocess.run(args, capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-600:] + r.stderr[-1200:]
    assert json.loads(r.stdout.strip().splitlines()[-1])["vcl"] == case["n"]
    lines = [ln.split(" ", 1) for ln in open(log).read().splitlines()]
    threads = sorted({t for t, rest in lines if rest.startswith("ks265_encode_picture")})
    assert len(threads) == 1, threads
    return [rest for t, rest in lines if t == threads[0]]


def digest(lines: list[str]) -> str:
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()
