"""CPU tier of the compressed .ply (include/gs_splat.h: "Compressed .ply"): the host evaluators -- the functions the kernels call, compiled
for the host -- against a numpy mirror of the rules the header spells out, written here; the encoder's logarithm against math.log; what a
splat loses on its way through a file and back, against the format's own quantisation step; and every header error.  No GPU anywhere.

The format is restated from memory of the published one: nothing here proves that a file of PlayCanvas' tools reads (docs/LAB_NOTES.md 9s)."""
import ctypes as C
import math

import numpy as np
import pytest

from conftest import load_case, pkg

capi = pkg("capi")

SH_C0 = 0.28209479177387814
SQRT2 = 1.4142135623730951
LN2 = 0.6931471805599453
CHUNK_NAMES = ["min_x", "min_y", "min_z", "max_x", "max_y", "max_z", "min_scale_x", "min_scale_y", "min_scale_z", "max_scale_x", "max_scale_y", "max_scale_z",
               "min_r", "min_g", "min_b", "max_r", "max_g", "max_b"]
VERTEX_NAMES = ["packed_position", "packed_rotation", "packed_scale", "packed_color"]
OTHERS = np.array([[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2]])


# ---------------------------------------------------------------- the mirror

def clamped_u8(v):
    """Uint8ClampedArray: NaN -> 0, clamp, round half to even"""
    v = np.asarray(v, np.float64)
    return np.where(np.isnan(v), 0.0, np.rint(np.clip(np.nan_to_num(v, nan=0.0), 0.0, 255.0))).astype(np.uint8)


def u(v, bits):
    m = (1 << bits) - 1
    return (np.asarray(v, np.uint32) & np.uint32(m)).astype(np.float64) / float(m)


def header(n, chunk_floats=18, per=0, chunks=None, sh_n=None):
    c = (n + 255) // 256 if chunks is None else chunks
    h = "ply\nformat binary_little_endian 1.0\nelement chunk %d\n" % c
    h += "".join("property float %s\n" % p for p in CHUNK_NAMES[:chunk_floats])
    h += "element vertex %d\n" % n + "".join("property uint %s\n" % p for p in VERTEX_NAMES)
    if per:
        h += "element sh %d\n" % (n if sh_n is None else sh_n) + "".join("property uchar f_rest_%d\n" % k for k in range(3 * per))
    return (h + "end_header\n").encode()


def split_file(data):
    """-> (header bytes, chunks f32[C, cf], packed u32[N, 4], sh bytes u8[N, 3 per], per)"""
    data = bytes(data)
    end = data.index(b"end_header\n") + 11
    info = capi.cply_info(data)
    n, c, cf = info["splats"], info["chunks"], info["chunk_floats"]
    per = {0: 0, 1: 3, 2: 8, 3: 15}[info["sh_degree"]]
    a = end + c * cf * 4
    chunks = np.frombuffer(data, "<f4", c * cf, end).reshape(c, cf)
    packed = np.frombuffer(data, "<u4", n * 4, a).reshape(n, 4)
    sh = np.frombuffer(data, np.uint8, n * 3 * per, a + n * 16).reshape(n, 3 * per)
    assert len(data) == a + n * 16 + n * 3 * per
    return data[:end], chunks, packed, sh, per


def mirror_decode(chunks, packed, sh, per):
    """-> dict(pos f32[N, 3], logscale f64[N, 3], qbytes, quat f64[N, 4] normalised, rgba, v f64[N, 3], sh f32[N, 3, K])"""
    n, cf = len(packed), chunks.shape[1] if len(chunks) else 18
    ch = chunks.astype(np.float64)[np.arange(n) >> 8] if n else np.zeros((0, cf))
    p, w, s, c = (packed[:, k] for k in range(4))

    def triple(word, lo, hi):
        t = np.stack([u(word >> np.uint32(21), 11), u(word >> np.uint32(11), 10), u(word, 11)], axis=1)
        return lo + (hi - lo) * t
    pos = triple(p, ch[:, 0:3], ch[:, 3:6]).astype(np.float32)
    logscale = triple(s, ch[:, 6:9], ch[:, 9:12])
    a, b, cc = ((u(w >> np.uint32(sh_), 10) - 0.5) * SQRT2 for sh_ in (20, 10, 0))
    m = np.sqrt(np.maximum(0.0, 1.0 - ((a * a + b * b) + cc * cc)))
    k = (w >> np.uint32(30)).astype(np.int64)
    q = np.zeros((n, 4))
    rest = np.stack([a, b, cc], axis=1)
    for i in range(4):
        sel = k == i
        q[sel, i] = m[sel]
        q[np.ix_(sel, OTHERS[i])] = rest[sel]
    ln = np.sqrt(((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3])
    q = q / ln[:, None]
    t = np.stack([u(c >> np.uint32(24), 8), u(c >> np.uint32(16), 8), u(c >> np.uint32(8), 8)], axis=1)
    v = ch[:, 12:15] + (ch[:, 15:18] - ch[:, 12:15]) * t if cf == 18 else t
    rgba = np.concatenate([clamped_u8(v * 255.0), clamped_u8(u(c, 8) * 255.0)[:, None]], axis=1)
    K = per + 1
    rows = np.zeros((n, 3, K), np.float32)
    rows[:, :, 0] = ((v - 0.5) / SH_C0).astype(np.float32)
    if per:
        rows[:, :, 1:] = (sh.reshape(n, 3, per).astype(np.float64) * (8.0 / 255.0) - 4.0).astype(np.float32)
    return dict(pos=pos, logscale=logscale, qbytes=clamped_u8(q * 128.0 + 128.0), quat=q, rgba=rgba, v=v, sh=rows)


def mirror_log_fixed(x):
    """the header's log_fixed on positive finite f64, operation for operation"""
    x = np.asarray(x, np.float64)
    m, e = np.frexp(x)                                            # m in [0.5, 1): exact, denormals included
    m = m * 2.0; e = e.astype(np.float64) - 1.0
    big = m >= SQRT2
    m = np.where(big, m * 0.5, m); e = np.where(big, e + 1.0, e)
    s = (m - 1.0) / (m + 1.0); z = s * s
    q = np.full_like(z, 1.0 / 21.0)
    for d in (19.0, 17.0, 15.0, 13.0, 11.0, 9.0, 7.0, 5.0, 3.0):
        q = 1.0 / d + z * q
    return e * LN2 + 2.0 * (s + s * (z * q))


def key(f):
    """ascending key = ascending value, -0 below +0"""
    b = np.asarray(f, np.float32).view(np.uint32)
    return np.where(b >> np.uint32(31), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def bounds(values):
    """(lo, hi) f32 over the finite entries of each column; none: 0, 0"""
    lo = np.zeros(values.shape[1], np.float32); hi = np.zeros(values.shape[1], np.float32)
    for j in range(values.shape[1]):
        col = values[:, j][np.isfinite(values[:, j])]
        if col.size:
            k = key(col)
            lo[j], hi[j] = col[np.argmin(k)], col[np.argmax(k)]
    return lo, hi


def code(t, bits):
    top = float((1 << bits) - 1)
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.floor(t * top + 0.5)
        out = np.where(np.isnan(t) | (t <= 0.0), 0.0, np.where(r >= top, top, r))
    return np.nan_to_num(out, nan=0.0).astype(np.uint32)


def frac(v, lo, hi):
    v, lo, hi = (np.asarray(a, np.float32).astype(np.float64) for a in (v, lo, hi))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return np.where(hi > lo, (v - lo) / np.where(hi > lo, hi - lo, 1.0), 0.0)


def spread(v):
    v = v.astype(np.uint32) & np.uint32(0x3FF)
    for sh_, mask in ((16, 0x030000FF), (8, 0x0300F00F), (4, 0x030C30C3), (2, 0x09249249)):
        v = (v | (v << np.uint32(sh_))) & np.uint32(mask)
    return v


def mirror_values(rows, wide, sh, sh_rows, K):
    n = len(rows)
    f = rows[:, :24].copy().view(np.float32).reshape(n, 6)
    val = np.zeros((n, 9), np.float32)
    val[:, 0:3] = f[:, 0:3]
    scale = (wide[:, 0:3] if wide is not None else f[:, 3:6]).astype(np.float64)
    good = scale > 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        lg = np.clip(mirror_log_fixed(np.where(good, scale, 1.0)), -20.0, 20.0)
    val[:, 3:6] = np.where(good, lg, -20.0).astype(np.float32)
    val[:, 6:9] = (rows[:, 24:27].astype(np.float64) / 255.0).astype(np.float32)
    if sh_rows:
        dc = sh.reshape(-1, 3, K)[:sh_rows, :, 0].astype(np.float64)
        val[:sh_rows, 6:9] = (0.5 + SH_C0 * dc).astype(np.float32)
    return val


def mirror_encode(rows, wide=None, sh=None, degree=0, morton=False):
    """-> (file bytes, order)"""
    rows = np.ascontiguousarray(rows, np.uint8).reshape(-1, 32)
    n, K = len(rows), (degree + 1) ** 2
    per = K - 1
    sh_rows = 0 if sh is None else len(sh)
    val = mirror_values(rows, wide, sh, sh_rows, K)
    order = np.arange(n)
    if morton and n:
        lo, hi = bounds(val[:, 0:3])
        t = frac(val[:, 0:3], lo[None, :], hi[None, :])
        with np.errstate(invalid="ignore"):
            ax = np.where(np.isnan(t) | (t < 0.0), 0.0, np.minimum(1023.0, np.floor(t * 1024.0)))
        ax = np.nan_to_num(ax, nan=0.0).astype(np.uint32)
        mc = spread(ax[:, 0]) | (spread(ax[:, 1]) << np.uint32(1)) | (spread(ax[:, 2]) << np.uint32(2))
        order = np.argsort(mc, kind="stable")
    q = wide[:, 3:7].astype(np.float64) if wide is not None else (rows[:, 28:32].astype(np.float64) - 128.0) / 128.0
    with np.errstate(invalid="ignore", over="ignore"):
        ln = np.sqrt(((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3])
        bad = ~(ln > 0.0) | ~(ln <= np.finfo(np.float64).max)
        q = np.where(bad[:, None], np.array([1.0, 0.0, 0.0, 0.0])[None, :], q / np.where(bad, 1.0, ln)[:, None])
    k = np.argmax(np.abs(q), axis=1)
    q = np.where((q[np.arange(n), k] < 0.0)[:, None], -q, q)
    oth = np.take_along_axis(q, OTHERS[k], axis=1) if n else np.zeros((0, 3))
    rc = code(oth / SQRT2 + 0.5, 10)
    rot = (k.astype(np.uint32) << np.uint32(30)) | (rc[:, 0] << np.uint32(20)) | (rc[:, 1] << np.uint32(10)) | rc[:, 2]
    chunks, packed = [], np.zeros((n, 4), np.uint32)
    for c0 in range(0, n, 256):
        idx = order[c0:c0 + 256]
        lo, hi = bounds(val[idx])
        chunks.append(np.concatenate([lo[0:3], hi[0:3], lo[3:6], hi[3:6], lo[6:9], hi[6:9]]))
        t = frac(val[idx], lo[None, :], hi[None, :])
        out = packed[c0:c0 + len(idx)]
        out[:, 0] = (code(t[:, 0], 11) << np.uint32(21)) | (code(t[:, 1], 10) << np.uint32(11)) | code(t[:, 2], 11)
        out[:, 1] = rot[idx]
        out[:, 2] = (code(t[:, 3], 11) << np.uint32(21)) | (code(t[:, 4], 10) << np.uint32(11)) | code(t[:, 5], 11)
        out[:, 3] = (code(t[:, 6], 8) << np.uint32(24)) | (code(t[:, 7], 8) << np.uint32(16)) | (code(t[:, 8], 8) << np.uint32(8)) | rows[idx, 27].astype(np.uint32)
    shb = np.full((n, 3, per), 128, np.uint8)
    if sh_rows and per:
        coded = clamped_u8((sh.reshape(-1, 3, K)[:, :, 1:].astype(np.float64) + 4.0) * (255.0 / 8.0))
        has = order < sh_rows
        shb[has] = coded[order[has]]
    body = b"".join(np.asarray(c, "<f4").tobytes() for c in chunks) + packed.astype("<u4").tobytes() + shb.tobytes()
    return header(n, 18, per) + body, order.astype(np.uint32)


# ---------------------------------------------------------------- inputs

def make_rows(n, seed, spread_=3.0):
    g = np.random.Generator(np.random.PCG64(seed))
    rows = np.zeros((n, 32), np.uint8)
    pos = (g.normal(size=(n, 3)) * spread_).astype(np.float32)
    scale = np.exp(g.normal(size=(n, 3)) * 1.2 - 3.0).astype(np.float32)
    rows[:, 0:12] = pos.view(np.uint8).reshape(n, 12)
    rows[:, 12:24] = scale.view(np.uint8).reshape(n, 12)
    rows[:, 24:28] = g.integers(0, 256, (n, 4))
    q = g.normal(size=(n, 4)); q /= np.sqrt((q * q).sum(axis=1))[:, None]
    rows[:, 28:32] = clamped_u8(q * 128.0 + 128.0)
    wide = np.concatenate([scale * np.float32(1.0009765625), q.astype(np.float32)], axis=1)
    return rows, np.ascontiguousarray(wide, np.float32)


def make_file(n, chunk_floats, per, seed):
    """a file of random words against random bounds"""
    g = np.random.Generator(np.random.PCG64(seed))
    c = (n + 255) // 256
    ch = np.zeros((c, 18), np.float32)
    lo = g.normal(size=(c, 3)) * 4.0
    ch[:, 0:3], ch[:, 3:6] = lo, lo + g.uniform(0.0, 5.0, (c, 3))
    slo = g.uniform(-12.0, -2.0, (c, 3))
    ch[:, 6:9], ch[:, 9:12] = slo, slo + g.uniform(0.0, 6.0, (c, 3))
    ch[:, 12:15], ch[:, 15:18] = g.uniform(-0.3, 0.2, (c, 3)), g.uniform(0.7, 1.4, (c, 3))      # colours beyond [0, 1]: the clamp
    packed = g.integers(0, 1 << 32, (n, 4), dtype=np.uint64).astype(np.uint32)
    sh = g.integers(0, 256, (n, 3 * per), dtype=np.uint8) if per else np.zeros((n, 0), np.uint8)
    ch = ch[:, :chunk_floats]
    return header(n, chunk_floats, per) + ch.astype("<f4").tobytes() + packed.astype("<u4").tobytes() + sh.tobytes()


def test_the_library_has_the_new_calls():
    L = capi.load()
    for name in ("gs_cply_info", "gs_cply_to_splat", "gs_cply_sh_host", "gs_splat_to_cply", "gs_log_fixed", "gs_load_cply", "gs_cply_to_splat_gpu",
                 "gs_export_cply", "gs_multi_load_cply", "gs_multi_export_cply"):
        assert hasattr(L, name) and name in capi.EXPORTS, name


# ---------------------------------------------------------------- decode

@pytest.mark.parametrize("chunk_floats,per", [(18, 0), (12, 0), (18, 3), (12, 8), (18, 15)])
def test_the_host_decoder_equals_the_mirror(chunk_floats, per):
    n = 513
    data = make_file(n, chunk_floats, per, seed=100 + chunk_floats + per)
    info = capi.cply_info(data)
    assert info == {"splats": n, "chunks": 3, "sh_degree": {0: 0, 3: 1, 8: 2, 15: 3}[per], "chunk_floats": chunk_floats}
    _, chunks, packed, sh, per2 = split_file(data)
    assert per2 == per
    want = mirror_decode(chunks, packed, sh, per)
    rows, wide = capi.cply_to_splat(data, want_wide=True)
    assert rows.shape == (n, 32) and np.array_equal(capi.cply_to_splat(data), rows)
    f = rows[:, :24].copy().view(np.float32).reshape(n, 6)
    assert np.array_equal(f[:, 0:3].view(np.uint32), want["pos"].view(np.uint32))
    assert np.array_equal(rows[:, 24:28], want["rgba"])
    assert np.array_equal(rows[:, 28:32], want["qbytes"])
    # js_exp is < 1 ulp f64 from exp: the f32 scale within one f32 ulp of numpy's
    ref = np.exp(want["logscale"]).astype(np.float32)
    ulps = np.abs(f[:, 3:6].view(np.int32).astype(np.int64) - ref.view(np.int32).astype(np.int64))
    assert ulps.max() <= 1, ulps.max()
    assert np.array_equal(wide[:, 0:3].view(np.uint32), f[:, 3:6].view(np.uint32))
    assert np.array_equal(wide[:, 3:7].view(np.uint32), want["quat"].astype(np.float32).view(np.uint32))
    for degree in range(4):
        got, d = capi.cply_sh(data, degree)
        D = min(degree, info["sh_degree"]); K = (D + 1) ** 2
        assert d == D and got.shape == (n, 3 * K)
        assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(want["sh"][:, :, :K]).reshape(n, 3 * K).view(np.uint32)), degree


def test_twelve_and_eighteen_float_chunks_differ_in_colour_only():
    n = 300
    d18 = make_file(n, 18, 0, seed=5)
    _, chunks, packed, _, _ = split_file(d18)
    d12 = header(n, 12, 0) + chunks[:, :12].astype("<f4").tobytes() + packed.astype("<u4").tobytes()
    r18, r12 = capi.cply_to_splat(d18), capi.cply_to_splat(d12)
    assert np.array_equal(r18[:, :24], r12[:, :24]) and np.array_equal(r18[:, 27:], r12[:, 27:])
    assert np.array_equal(r12[:, 24:27], clamped_u8(np.stack([u(packed[:, 3] >> np.uint32(s), 8) for s in (24, 16, 8)], axis=1) * 255.0))
    assert not np.array_equal(r18[:, 24:27], r12[:, 24:27])


# ---------------------------------------------------------------- encode

@pytest.mark.parametrize("degree", [0, 1, 2, 3])
@pytest.mark.parametrize("morton", [False, True])
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 513])
def test_the_host_encoder_equals_the_mirror(n, morton, degree):
    rows, wide = make_rows(n, seed=900 + n)
    g = np.random.Generator(np.random.PCG64(n * 8 + degree))
    sh_rows = (2 * n) // 3                                         # fewer SH rows than rows (0 of 0 and of 1)
    sh = (g.normal(size=(sh_rows, 3 * (degree + 1) ** 2)) * 1.5).astype(np.float32)      # (some beyond [-4, 4]: the clamp)
    for w in (None, wide):
        for s in (None, sh):
            want, order = mirror_encode(rows, w, s, degree, morton)
            got, index = capi.splat_to_cply(rows, w, s, degree, morton=morton, want_index=True)
            assert np.array_equal(index, order), (n, morton, degree)
            assert bytes(got) == want, (n, morton, degree, w is None, s is None)
    if morton and n > 256:
        assert not np.array_equal(order, np.arange(n))


def test_morton_ties_keep_the_input_order_and_chunks_shrink():
    n = 1000
    rows, wide = make_rows(n, seed=77)
    rows[500:520, 0:12] = rows[100, 0:12]                          # twenty splats at one position: one code
    data, index = capi.splat_to_cply(rows, wide, morton=True, want_index=True)
    assert sorted(index.tolist()) == list(range(n))
    at = [int(np.flatnonzero(index == i)[0]) for i in [100] + list(range(500, 520))]
    assert at == list(range(at[0], at[0] + 21))
    _, ch_m, _, _, _ = split_file(data)
    _, ch_0, _, _, _ = split_file(capi.splat_to_cply(rows, wide))
    vol = lambda ch: np.prod(ch[:, 3:6].astype(np.float64) - ch[:, 0:3], axis=1).sum()
    # the point of the order: in input order every chunk's box is about the scene's; a run of the curve never spans more than the scene
    assert vol(ch_m) < vol(ch_0)


def test_edge_inputs():
    n = 260
    rows, wide = make_rows(n, seed=31)
    f = rows[:, :24].view(np.float32).reshape(n, 6)
    f[256:, 0:3] = (1.5, -2.0, 0.25)                               # the second chunk: zero extent
    wide[0, 3:7] = 0.0                                             # a zero quaternion
    wide[1, 3:7] = (np.inf, 0.0, 0.0, 1.0)                         # ... and one that is not finite
    for i in range(4):                                             # the largest component at each index, negative
        qq = np.full(4, 0.2, np.float32); qq[i] = -0.9; qq[(i + 1) % 4] = -0.1
        wide[2 + i, 3:7] = qq
    wide[6, 3:7] = (0.5, -0.5, 0.5, -0.5)                          # a tie: the first index wins
    wide[7, 0:3] = (0.0, -1.0, np.nan)                             # scales without a logarithm
    f[8, 0] = np.nan                                               # a position that takes no part in the bounds
    f[9, 1] = np.inf
    for morton in (False, True):
        want, order = mirror_encode(rows, wide, None, 0, morton)
        got, index = capi.splat_to_cply(rows, wide, morton=morton, want_index=True)
        assert np.array_equal(index, order) and bytes(got) == want, morton
    data = capi.splat_to_cply(rows, wide)
    _, chunks, packed, _, _ = split_file(data)
    assert np.array_equal(chunks[1, 0:3], chunks[1, 3:6]) and (packed[256:, 0] == 0).all()
    assert np.isfinite(chunks).all() and packed[8, 0] >> 21 == 0 and (packed[9, 0] >> 11) & 1023 == 1023
    assert packed[0, 1] == packed[1, 1] == (512 << 20 | 512 << 10 | 512)            # (1, 0, 0, 0): k = 0, three centres
    assert [int(packed[2 + i, 1] >> 30) for i in range(4)] == [0, 1, 2, 3] and packed[6, 1] >> 30 == 0
    assert chunks[0, 6] == chunks[0, 7] == chunks[0, 8] == -20.0 and packed[7, 2] == 0
    back, bw = capi.cply_to_splat(data, want_wide=True)
    fb = back[:, :24].copy().view(np.float32).reshape(n, 6)
    assert np.array_equal(fb[256:, 0:3], f[256:, 0:3])                              # zero extent: the bound itself comes back
    assert np.array_equal(back[0, 28:32], [255, 128, 128, 128])
    for i in range(4):                                                              # q and -q are one rotation: the largest comes back positive
        qn = -wide[2 + i, 3:7].astype(np.float64); qn /= np.sqrt((qn * qn).sum())
        assert np.abs(bw[2 + i, 3:7] - qn).max() <= SQRT2 / 1023 + 1e-6


# ---------------------------------------------------------------- the logarithm

def test_log_fixed_against_math_log():
    """relative error <= 4e-16 (what was measured: docs/LAB_NOTES.md 9s)"""
    grid = np.concatenate([10.0 ** np.linspace(-300.0, 300.0, 10000), [5e-324, 1e-320, 2.5e-310, 2.2250738585072014e-308, 1.0, 2.0, 0.5, SQRT2, 1.7976931348623157e308],
                           1.0 + np.linspace(-0.3, 0.45, 501)])
    worst = 0.0
    for x in grid:
        got, want = capi.log_fixed(float(x)), math.log(float(x))
        if want == 0.0:
            assert got == 0.0
            continue
        worst = max(worst, abs(got - want) / abs(want))
    print("gs_log_fixed: worst relative error %.3g over %d arguments" % (worst, grid.size))
    assert worst <= 4e-16
    assert np.array_equal(np.array([capi.log_fixed(float(x)) for x in grid[::37]]), mirror_log_fixed(grid[::37]))
    assert capi.log_fixed(0.0) == -math.inf and math.isnan(capi.log_fixed(-1.0)) and math.isnan(capi.log_fixed(math.nan)) and capi.log_fixed(math.inf) == math.inf


# ---------------------------------------------------------------- round trip

@pytest.mark.parametrize("morton", [False, True])
def test_encode_then_decode_is_within_the_quantisation_step(morton):
    n, degree = 1000, 2
    rows, wide = make_rows(n, seed=4242)
    g = np.random.Generator(np.random.PCG64(6))
    sh = (g.normal(size=(600, 27)) * 0.4).astype(np.float32)
    data, index = capi.splat_to_cply(rows, wide, sh, degree, morton=morton, want_index=True)
    _, chunks, _, _, _ = split_file(data)
    back = capi.cply_to_splat(data)
    src = rows[index]
    pos, got = src[:, :12].copy().view(np.float32).reshape(n, 3), back[:, :12].copy().view(np.float32).reshape(n, 3)
    ch = chunks.astype(np.float64)[np.arange(n) >> 8]
    for axis, bits in ((0, 11), (1, 10), (2, 11)):
        lo, hi = ch[:, axis], ch[:, 3 + axis]
        bound = 0.5 * (hi - lo) / ((1 << bits) - 1) * (1.0 + 2.0 ** -20) + np.spacing(np.maximum(np.abs(lo), np.abs(hi)).astype(np.float32)).astype(np.float64)
        err = np.abs(got[:, axis].astype(np.float64) - pos[:, axis].astype(np.float64))
        assert (err <= bound).all(), (axis, float((err / bound).max()))
    assert np.array_equal(back[:, 27], src[:, 27])                                   # the alpha byte is exact
    no_sh = index >= 600
    assert np.abs(back[no_sh, 24:27].astype(int) - src[no_sh, 24:27].astype(int)).max() <= 1
    # the scales: half a step of the log-scale code, and what the f32 roundings add
    ws = wide[index, 0:3].astype(np.float64)
    gs_ = back[:, 12:24].copy().view(np.float32).reshape(n, 3).astype(np.float64)
    step = np.stack([(ch[:, 9 + a] - ch[:, 6 + a]) / ((1 << b) - 1) for a, b in ((0, 11), (1, 10), (2, 11))], axis=1)
    assert (np.abs(np.log(gs_) - np.log(ws)) <= 0.5 * step * (1.0 + 2.0 ** -20) + 4e-6).all()
    # the SH rows of the splats that have one: DC within half a colour step, the rest within half a byte step
    rows_sh, d = capi.cply_sh(data, 3)
    assert d == degree
    has = np.flatnonzero(index < 600)
    a, b = rows_sh.reshape(n, 3, 9)[has], sh.reshape(600, 3, 9)[index[has]]
    assert np.abs(a[:, :, 1:] - b[:, :, 1:]).max() <= 0.5 * 8.0 / 255.0 + 1e-6
    cstep = (ch[has, 15:18] - ch[has, 12:15]) / 255.0 / SH_C0
    assert (np.abs(a[:, :, 0].astype(np.float64) - b[:, :, 0]) <= 0.5 * cstep * (1.0 + 2.0 ** -20) + 1e-6).all()
    assert np.array_equal(rows_sh.reshape(n, 3, 9)[~np.isin(np.arange(n), has)][:, :, 1:], np.zeros((n - has.size, 3, 8), np.float32) + np.float32(128 * (8.0 / 255.0) - 4.0))


# ---------------------------------------------------------------- the header

def expect(data, code_, word=None):
    with pytest.raises(capi.GsError) as e:
        capi.cply_info(data)
    assert e.value.code == code_, (e.value.code, str(e.value))
    assert str(e.value) and (word is None or word in str(e.value)), str(e.value)
    for call in (capi.cply_to_splat, capi.cply_sh):
        with pytest.raises(capi.GsError) as e2:
            call(data)
        assert e2.value.code == code_


def test_every_header_error():
    n = 300
    good = make_file(n, 18, 3, seed=1)
    body = good[good.index(b"end_header\n") + 11:]
    assert capi.cply_info(good)["splats"] == n
    assert capi.cply_info(good.replace(b"element chunk", b"comment written by a test\nelement chunk").replace(b"end_header", b"comment x\nend_header", 1))["splats"] == n
    H = capi.E_PLY_HEADER
    expect(good.replace(b"min_scale_y", b"min_scale_w"), H, "min_scale_y")                       # another name
    expect(good.replace(b"property float max_z", b"property double max_z"), H)                    # another type
    expect(good.replace(b"property uint packed_scale", b"property int packed_scale"), H, "packed_scale")
    expect(good.replace(b"property uchar f_rest_4\n", b"property char f_rest_4\n"), H)
    expect(good.replace(b"property float min_x\nproperty float min_y\n", b"property float min_y\nproperty float min_x\n"), H)     # another order
    expect(good.replace(b"property uint packed_rotation\nproperty uint packed_scale\n", b"property uint packed_scale\nproperty uint packed_rotation\n"), H)
    expect(good.replace(b"property float max_b\n", b""), H)                                      # another count: 17 chunk floats
    expect(good.replace(b"property uint packed_color\n", b""), H)
    expect(good.replace(b"property uchar f_rest_8\n", b""), H)                                   # 8 f_rest
    expect(header(n, 18, 3).replace(b"end_header\n", b"property uchar f_rest_9\nend_header\n") + body, H)
    expect(header(n, 18, 0).replace(b"end_header\n", b"property float extra\nend_header\n") + body, H)
    expect(header(n, 18, 3, chunks=1) + body, H, "256")                                          # C wrong
    expect(header(n, 18, 3, chunks=3) + body, H, "256")
    expect(header(n, 18, 3, sh_n=n - 1) + body, H)                                               # sh count != N
    expect(good.replace(b"binary_little_endian", b"binary_big_endian"), H)
    expect(good.replace(b"binary_little_endian 1.0", b"ascii 1.0"), H)
    expect(b"plx" + good[3:], H)
    expect(good.replace(b"end_header\n", b"end_header \n"), H)
    # the vertex element first: an INRIA file -- the sniff
    inria = bytes(load_case("ply_inria64")["ply"])
    assert capi.ply_to_splat(inria).size == 64 * 32
    expect(inria, H, "element chunk")
    # a body shorter than the header promises
    expect(good[:-1], capi.E_PLY_DATA)
    expect(header(n, 18, 3), capi.E_PLY_DATA)
    assert capi.cply_to_splat(good + b"tail").shape == (n, 32)                                   # (a longer one is read)
    # the writer's bad arguments
    nb = C.c_size_t(0)
    L = capi.load()
    rows, _ = make_rows(4, seed=2)
    assert L.gs_splat_to_cply(capi._p(rows), None, None, 0, 0, 4, 2, None, None, C.byref(nb)) == capi.E_BADARG          # an unknown flag
    assert L.gs_splat_to_cply(capi._p(rows), None, None, 0, 4, 4, 0, None, None, C.byref(nb)) == capi.E_BADARG
    assert L.gs_splat_to_cply(capi._p(rows), None, None, 5, 1, 4, 0, None, None, C.byref(nb)) == capi.E_BADARG
    assert L.gs_splat_to_cply(capi._p(rows), None, None, 0, 0, 4, 0, None, None, None) == capi.E_BADARG
    assert L.gs_log_fixed(1.0, None) == capi.E_BADARG
