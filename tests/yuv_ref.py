"""Planar Y'CbCr frames <-> HWC float RGB, restated in float32 numpy operation for operation (DESIGN.md §9;
include/nlk_hip.h: nlk_dev_yuv_to_rgb / nlk_dev_rgb_to_yuv): the bit-for-bit reference of the two kernels. Every
intermediate is a float32 array and every line below is one rounding, in the kernels' order (they are compiled without
contraction and do not divide). Plus a small YUV4MPEG2 reader and writer for the tool's tests."""
from types import SimpleNamespace

import numpy as np

F = np.float32


def fmt(tag=None, full_range=False, matrix=709):
    """The format of a y4m `C` tag value (None / "" = absent), as nlk_yuv_format_from_tag maps it; ValueError for
    what that refuses."""
    t = tag or "420jpeg"
    depth, base = 8, t
    for fam in ("420p", "422p", "444p", "mono"):
        if t.startswith(fam) and t[len(fam):].isdigit() and t != fam:
            depth, base = int(t[len(fam):]), fam.rstrip("p")
            if not (9 <= depth <= 16 and str(depth) == t[len(fam):]):
                raise ValueError(tag)
    table = {"420jpeg": (0, 2, 2, 0), "420mpeg2": (0, 2, 2, 1), "420": (0, 2, 2, 1), "422": (0, 2, 1, 1),
             "444": (0, 1, 1, 0), "mono": (1, 1, 1, 0)}
    if base not in table or (depth > 8 and base in ("420jpeg", "420mpeg2")):
        raise ValueError(tag)
    mono, sx, sy, cos = table[base]
    return SimpleNamespace(mono=mono, sx=sx, sy=sy, cosited_x=cos, depth=depth, full_range=int(bool(full_range)),
                           matrix=int(matrix))


def chroma_size(w, h, f):
    return (w + f.sx - 1) // f.sx, (h + f.sy - 1) // f.sy


def frame_bytes(w, h, f):
    cw, chh = chroma_size(w, h, f)
    return (w * h + (0 if f.mono else 2 * cw * chh)) * (2 if f.depth > 8 else 1)


def constants(f):
    """The constants, in double (Python floats) in the host code's expression order, each rounded to float32 once."""
    s, top = float(1 << (f.depth - 8)), float((1 << f.depth) - 1)
    y0, c0 = (0.0 if f.full_range else 16.0 * s), 128.0 * s
    ky = 255.0 / top if f.full_range else 255.0 / (219.0 * s)
    kc = 255.0 / top if f.full_range else 255.0 / (224.0 * s)
    kr, kb = (0.299, 0.114) if f.matrix == 601 else (0.2126, 0.0722)
    kg = 1.0 - kr - kb
    crr, cbu = 2.0 * (1.0 - kr), 2.0 * (1.0 - kb)
    cgu, cgv = 2.0 * kb * (1.0 - kb) / kg, 2.0 * kr * (1.0 - kr) / kg
    k = dict(y0=y0, ky=ky, c0=c0, kc=kc, crr=crr, cbu=cbu, cgu=cgu, cgv=cgv, kr=kr, kg=kg, kb=kb, icbu=1.0 / cbu,
             icrr=1.0 / crr, iky=1.0 / ky, ikc=1.0 / kc, maxc=top)
    return SimpleNamespace(**{n: F(v) for n, v in k.items()})


def split(payload, w, h, f):
    """(Y, Cb, Cr) code planes (Cb = Cr = None for mono) of one frame's bytes."""
    a = np.frombuffer(bytes(payload), np.uint8)
    assert a.size == frame_bytes(w, h, f), (a.size, frame_bytes(w, h, f))
    s = a.view("<u2") if f.depth > 8 else a
    Y = s[:w * h].reshape(h, w)
    if f.mono:
        return Y, None, None
    cw, chh = chroma_size(w, h, f)
    return Y, s[w * h:w * h + cw * chh].reshape(chh, cw), s[w * h + cw * chh:].reshape(chh, cw)


def join(Y, Cb, Cr, f):
    dt = "<u2" if f.depth > 8 else np.uint8
    planes = [Y] if f.mono else [Y, Cb, Cr]
    return np.concatenate([np.ascontiguousarray(p).astype(dt).ravel().view(np.uint8) for p in planes])


def _up(c, n, axis, cosited):
    """A chroma plane interpolated to the n luma positions of `axis` (subsampled by 2), indices clamped."""
    c = np.moveaxis(c, axis, 0)
    x = np.arange(n)
    i = x >> 1
    last = c.shape[0] - 1
    if cosited:      # even: the sample; odd: the mean of two
        mean = (c[i] + c[np.minimum(i + 1, last)]) * F(0.5)
        odd = (x & 1).astype(bool).reshape((-1,) + (1,) * (c.ndim - 1))
        out = np.where(odd, mean, c[i])
    else:            # 3/4 near + 1/4 far: far = i - 1 left of an even position, i + 1 right of an odd one
        far = np.clip(np.where(x & 1, i + 1, i - 1), 0, last)
        out = F(0.75) * c[i] + F(0.25) * c[far]
    return np.moveaxis(out.astype(F), 0, axis)


def to_rgb(payload, w, h, f):
    k = constants(f)
    Y, Cb, Cr = split(payload, w, h, f)
    y = (Y.astype(F) - k.y0) * k.ky
    if f.mono:
        return y[:, :, None]
    uv = []
    for P in (Cb, Cr):
        c = (P.astype(F) - k.c0) * k.kc
        if f.sx == 2:
            c = _up(c, w, 1, bool(f.cosited_x))      # inside a chroma row first ...
        if f.sy == 2:
            c = _up(c, h, 0, False)                  # ... then across the rows (always centred)
        uv.append(c)
    u, v = uv
    R = y + k.crr * v
    G = (y - k.cgu * u) - k.cgv * v
    B = y + k.cbu * u
    return np.stack([R, G, B], -1).astype(F)


def _down(p, axis, cosited):
    """A luma-resolution plane decimated by 2 along `axis`, indices clamped."""
    p = np.moveaxis(p, axis, 0)
    n = p.shape[0]
    i2 = 2 * np.arange((n + 1) // 2)
    nxt = np.minimum(i2 + 1, n - 1)
    if cosited:
        out = (F(0.25) * p[np.maximum(i2 - 1, 0)] + F(0.5) * p[i2]) + F(0.25) * p[nxt]
    else:
        out = (p[i2] + p[nxt]) * F(0.5)
    return np.moveaxis(out.astype(F), 0, axis)


def _code(v, ik, off, maxc, depth):
    with np.errstate(invalid="ignore"):
        t = np.rint(v * ik + off)                     # to nearest even
        t = np.where(np.isnan(t), F(0), np.clip(t, F(0), maxc))
    return t.astype(np.uint16 if depth > 8 else np.uint8)


def to_yuv(rgb, f):
    """One frame's bytes (uint8 array) from the (h, w, ch) float32 image."""
    k = constants(f)
    a = np.asarray(rgb, F)
    if a.ndim == 2:
        a = a[:, :, None]
    if f.mono:
        return join(_code(a[:, :, 0], k.iky, k.y0, k.maxc, f.depth), None, None, f)
    with np.errstate(invalid="ignore", over="ignore"):
        R, G, B = a[:, :, 0], a[:, :, 1], a[:, :, 2]
        y = (k.kr * R + k.kg * G) + k.kb * B
        u = (B - y) * k.icbu
        v = (R - y) * k.icrr
        planes = []
        for p in (u, v):
            if f.sx == 2:
                p = _down(p, 1, bool(f.cosited_x))   # along the luma rows 2j and min(2j + 1, h - 1) first ...
            if f.sy == 2:
                p = _down(p, 0, False)               # ... then (a + b) / 2 of the two
            planes.append(_code(p, k.ikc, k.c0, k.maxc, f.depth))
    return join(_code(y, k.iky, k.y0, k.maxc, f.depth), planes[0], planes[1], f)


# ---------------------------------------------------------------- the container

def y4m_header(w, h, tag=None, extra=""):
    """The header line (bytes, newline included); `extra`: further tags, e.g. " XCOLORRANGE=FULL"."""
    return ("YUV4MPEG2 W%d H%d F25:1 Ip A1:1%s%s\n" % (w, h, " C" + tag if tag else "", extra)).encode()


def y4m_bytes(w, h, tag, payloads, extra=""):
    return y4m_header(w, h, tag, extra) + b"".join(b"FRAME\n" + bytes(p) for p in payloads)


def y4m_parse(data):
    """(header line, w, h, C tag or None, [payload bytes]) of a well-formed stream."""
    nl = data.index(b"\n")
    line, tags = data[:nl + 1], data[:nl].split(b" ")
    assert tags[0] == b"YUV4MPEG2"
    d = {t[:1]: t[1:].decode() for t in tags[1:] if t[:1] in b"WHC"}
    w, h, tag = int(d[b"W"]), int(d[b"H"]), d.get(b"C")
    n = frame_bytes(w, h, fmt(tag))
    frames, at = [], nl + 1
    while at < len(data):
        e = data.index(b"\n", at)
        assert data[at:at + 5] == b"FRAME", data[at:at + 16]
        frames.append(data[e + 1:e + 1 + n])
        assert len(frames[-1]) == n
        at = e + 1 + n
    return line, w, h, tag, frames
