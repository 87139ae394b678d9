"""CPU tier of the view-dependent colour (GS_OPT_SH_DEGREE, csrc/gs_sh.h): the arithmetic against a numpy f64 mirror written here
(bit for bit), the basis against associated Legendre polynomials, degree 0 against the reference's baked bytes, the row order of
gs_ply_sh against the oracle's converter, the header rules and gs_camera_in_object.

The mirror (`sh_mirror`) restates the header: the same IEEE f64 operations in the same order, vectorised over splats.  numpy's
+ - * / sqrt on float64 are the correctly rounded machine operations, so no tolerance applies.  The GPU tier imports it."""
import math

import numpy as np
import pytest

from conftest import load_case, pkg
from oracle import oracle

capi = pkg("capi")
synth = pkg("synth")

SH_C0 = 0.28209479177387814
SH_C1 = 0.4886025119029199
SH_C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
SH_C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658, 1.445305721320277,
         -0.5900435899266435)


def clamped_u8(v):
    """Uint8ClampedArray store: clamp, round half to even, NaN -> 0 (csrc/gs_ply.h)."""
    v = np.asarray(v, np.float64)
    with np.errstate(invalid="ignore"):
        f = np.floor(v)
        d = v - f
        up = (d > 0.5) | ((d == 0.5) & (np.mod(f, 2.0) == 1.0))
        r = np.where(up, f + 1.0, f)
        r = np.where(v >= 255.0, 255.0, r)
        r = np.where(v > 0.0, r, 0.0)                  # also NaN
    return r.astype(np.uint8)


def sh_mirror(sh, degree, cam, pos, unrounded=False):
    """sh: (n, 3, K) f32 with K >= (degree+1)^2, cam: f64 x3, pos: (n, 3) f32 -> (n, 3) bytes (or the f64 values before rounding)."""
    sh = np.asarray(sh, np.float32).astype(np.float64)
    pos = np.asarray(pos, np.float32).astype(np.float64).reshape(-1, 3)
    cam = np.asarray(cam, np.float64).reshape(3)
    with np.errstate(all="ignore"):
        dx, dy, dz = pos[:, 0] - cam[0], pos[:, 1] - cam[1], pos[:, 2] - cam[2]
        ln = np.sqrt((dx * dx + dy * dy) + dz * dz)
        nz = ln != 0.0
        safe = np.where(nz, ln, 1.0)
        x, y, z = np.where(nz, dx / safe, 0.0), np.where(nz, dy / safe, 0.0), np.where(nz, dz / safe, 0.0)
        r = 0.5 + SH_C0 * sh[:, :, 0]

        def term(k, b):
            nonlocal r
            r = r + b[:, None] * sh[:, :, k]
        if degree >= 1:
            term(1, -SH_C1 * y); term(2, SH_C1 * z); term(3, -SH_C1 * x)
        if degree >= 2:
            xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
            term(4, SH_C2[0] * xy); term(5, SH_C2[1] * yz); term(6, SH_C2[2] * ((2.0 * zz - xx) - yy))
            term(7, SH_C2[3] * xz); term(8, SH_C2[4] * (xx - yy))
        if degree >= 3:
            term(9, (SH_C3[0] * y) * (3.0 * xx - yy)); term(10, (SH_C3[1] * xy) * z)
            term(11, (SH_C3[2] * y) * ((4.0 * zz - xx) - yy)); term(12, (SH_C3[3] * z) * ((2.0 * zz - 3.0 * xx) - 3.0 * yy))
            term(13, (SH_C3[4] * x) * ((4.0 * zz - xx) - yy)); term(14, (SH_C3[5] * z) * (xx - yy))
            term(15, (SH_C3[6] * x) * (xx - 3.0 * yy))
        v = r * 255
    return v if unrounded else clamped_u8(v)


def lib_eval(sh, degree, cam, pos, unrounded=False):
    """gs_sh_eval row by row: sh (n, 3, K) with K == (degree+1)^2."""
    return np.stack([capi.sh_eval(sh[i].reshape(-1), degree, cam, pos[i], unrounded=unrounded) for i in range(len(sh))])


def random_rows(n, degree, seed, spread=2.0):
    g = np.random.default_rng(seed)
    K = (degree + 1) ** 2
    sh = (g.standard_normal((n, 3, K)) * spread).astype(np.float32)        # 0.5 + 0.28 * (+-6) and beyond: past both clamps
    pos = (g.standard_normal((n, 3)) * 3).astype(np.float32)
    return sh, pos


# ---------------------------------------------------------------- 1. arithmetic

@pytest.mark.parametrize("degree", [0, 1, 2, 3])
def test_mirror_equals_library_bit_for_bit(degree):
    sh, pos = random_rows(600, degree, 100 + degree)
    for cam in ([0.0, 0.0, 0.0], [1.25, -3.5, 0.75], [1e-3, 2e5, -7.0]):
        got, want = lib_eval(sh, degree, cam, pos), sh_mirror(sh, degree, cam, pos)
        assert np.array_equal(got, want)
        gu, wu = lib_eval(sh, degree, cam, pos, unrounded=True), sh_mirror(sh, degree, cam, pos, unrounded=True)
        assert np.array_equal(gu.view(np.uint64), wu.view(np.uint64))      # the f64 values themselves, not only the bytes
    b = sh_mirror(sh, degree, [0, 0, 0], pos)
    assert (b == 0).any() and (b == 255).any() and ((b > 0) & (b < 255)).any()   # the inputs reach past the clamp on both sides


def test_half_ties_round_to_even_at_degree_0():
    # (0.5 + SH_C0 * dc) * 255 is exactly b + 0.5 only where SH_C0 * dc vanishes against 0.5 -- f32 spacing times 72 is 1e8 times the
    # f64 spacing of the result -- so the exact ties an f32 coefficient can reach all sit at 127.5: zeros, denormals, anything tiny
    one = np.ones((1, 3), np.float32)
    for t in (0.0, -0.0, 1e-45, -1e-45, 1e-30, -1e-30, 1e-18, -1e-18):
        assert (0.5 + SH_C0 * float(np.float32(t))) * 255 == 127.5
        sh = np.full((1, 3, 1), t, np.float32)
        assert lib_eval(sh, 0, [0, 0, 0], one)[0].tolist() == [128, 128, 128]                # half to even, not down
        assert sh_mirror(sh, 0, [0, 0, 0], one)[0].tolist() == [128, 128, 128]
    # ... and around every other b + 0.5 the nearest f32 coefficients on both sides: decided like Python's exact round()
    near = []
    for b in range(0, 255):
        t = np.float32(((b + 0.5) / 255.0 - 0.5) / SH_C0)
        for _ in range(4):
            t = np.nextafter(t, np.float32(-np.inf))
        for _ in range(9):
            near.append(t)
            t = np.nextafter(t, np.float32(np.inf))
    sh = np.repeat(np.array(near, np.float32).reshape(-1, 1, 1), 3, axis=1)
    pos = np.ones((len(near), 3), np.float32)
    got = lib_eval(sh, 0, [0, 0, 0], pos)
    want = [min(255, max(0, round((0.5 + SH_C0 * float(t)) * 255))) for t in near]
    assert got[:, 0].tolist() == want and np.array_equal(got, sh_mirror(sh, 0, [0, 0, 0], pos))
    assert len(set(want)) == 256


@pytest.mark.parametrize("degree", [0, 1, 2, 3])
def test_nan_inf_coefficients_and_splat_at_the_camera(degree):
    sh, pos = random_rows(64, degree, 7)
    K = sh.shape[2]
    sh[0, 0, 0] = np.nan; sh[1, 1, K - 1] = np.inf; sh[2, 2, K // 2] = -np.inf; sh[3, :, :] = np.nan; sh[4, 0, 0] = np.inf; sh[5, 0, 0] = -np.inf
    cam = np.array([0.5, -0.25, 2.0])
    pos[10:20] = cam.astype(np.float32)                                        # |pos - cam| == 0: d = (0, 0, 0)
    got, want = lib_eval(sh, degree, cam, pos), sh_mirror(sh, degree, cam, pos)
    assert np.array_equal(got, want)
    assert got[0, 0] == 0 and got[3].tolist() == [0, 0, 0] and got[4, 0] == 255 and got[5, 0] == 0
    dc_only = clamped_u8((0.5 + SH_C0 * sh[10:20, :, 0].astype(np.float64)) * 255)
    assert np.array_equal(got[10:20], dc_only)                                 # only the DC term survives at the camera


def test_zero_higher_bands_give_the_baked_byte():
    sh, pos = random_rows(300, 3, 11, spread=1.0)
    sh[:, :, 1:] = 0.0
    baked = clamped_u8((0.5 + SH_C0 * sh[:, :, 0].astype(np.float64)) * 255)
    for degree in (1, 2, 3):
        K = (degree + 1) ** 2
        assert np.array_equal(lib_eval(np.ascontiguousarray(sh[:, :, :K]), degree, [3.0, 1.0, -2.0], pos), baked)


# ---------------------------------------------------------------- 2. the basis, a second way

def _legendre(l, m, x):
    """Associated Legendre P_l^m(x) with the Condon-Shortley phase, by the standard recurrences."""
    pmm = 1.0
    if m > 0:
        s = math.sqrt((1.0 - x) * (1.0 + x))
        f = 1.0
        for _ in range(m):
            pmm *= -f * s
            f += 2.0
    if l == m:
        return pmm
    pm1 = x * (2 * m + 1) * pmm
    if l == m + 1:
        return pm1
    for ll in range(m + 2, l + 1):
        pll = (x * (2 * ll - 1) * pm1 - (ll + m - 1) * pmm) / (ll - m)
        pmm, pm1 = pm1, pll
    return pm1


def _real_sh(l, m, theta, phi):
    """Real spherical harmonic in the sign convention of the published eval_sh: N_l|m| P_l^|m|(cos theta) (phase included) times
    sqrt 2 cos(m phi) (m > 0), 1 (m = 0), sqrt 2 sin(|m| phi) (m < 0)."""
    a = abs(m)
    n = math.sqrt((2 * l + 1) / (4 * math.pi) * math.factorial(l - a) / math.factorial(l + a))
    p = _legendre(l, a, math.cos(theta))
    if m == 0:
        return n * p
    return math.sqrt(2.0) * n * p * (math.cos(m * phi) if m > 0 else math.sin(a * phi))


def test_basis_against_associated_legendre_polynomials():
    g = np.random.default_rng(5)
    worst = 0.0
    for _ in range(200):
        d = g.standard_normal(3)
        d /= np.linalg.norm(d)
        theta, phi = math.acos(max(-1.0, min(1.0, d[2]))), math.atan2(d[1], d[0])
        sh = g.standard_normal((1, 3, 16)).astype(np.float32)
        cam = g.standard_normal(3) * 2
        dist = 2.0 ** int(g.integers(-2, 3))                                    # pos = cam + dist * d (then rounded to f32)
        pos = (cam + dist * d).astype(np.float32).reshape(1, 3)
        dd = pos[0].astype(np.float64) - cam
        dd /= np.linalg.norm(dd)
        theta, phi = math.acos(max(-1.0, min(1.0, dd[2]))), math.atan2(dd[1], dd[0])
        for degree in (1, 2, 3):
            K = (degree + 1) ** 2
            want = np.zeros(3)
            for c in range(3):
                acc, k = 0.5, 0
                for l in range(degree + 1):
                    for m in range(-l, l + 1):
                        acc += _real_sh(l, m, theta, phi) * float(sh[0, c, k])
                        k += 1
                want[c] = acc * 255
            got = capi.sh_eval(np.ascontiguousarray(sh[0, :, :K]).reshape(-1), degree, cam, pos[0], unrounded=True)
            mir = sh_mirror(sh[:, :, :K], degree, cam, pos, unrounded=True)[0]
            worst = max(worst, float(np.abs(got - want).max()), float(np.abs(mir - want).max()))
    print("largest |header - Legendre| = %.3e colour bytes" % worst)
    assert worst <= 1e-9


# ---------------------------------------------------------------- 3. degree 0 is the reference

@pytest.mark.parametrize("name", ["ply_inria64", "ply_n4096"])
def test_degree_0_reproduces_the_golden_rgb(name):
    case = load_case(name)
    rows = case["rows"].reshape(-1, 32)
    sh, d = capi.ply_sh(bytes(case["ply"]), 0)
    assert d == 0 and sh.shape == (len(rows), 3)
    pos = rows[:, 0:12].copy().view("<f4").reshape(-1, 3)
    for cam in ([0, 0, 0], [4.0, -1.0, 2.5], pos[3].astype(np.float64)):
        got = lib_eval(sh.reshape(-1, 3, 1), 0, cam, pos)
        assert np.array_equal(got, rows[:, 24:27])
    full, dfull = capi.ply_sh(bytes(case["ply"]), 3)
    assert dfull == (3 if name == "ply_inria64" else 0)
    K = (dfull + 1) ** 2
    assert np.array_equal(full.reshape(-1, 3, K)[:, :, 0], sh)                 # k = 0 of every channel is f_dc_c


# ---------------------------------------------------------------- 4. order

def _header(ply):
    end = ply.index(b"end_header\n") + 11
    props, off = {}, 0
    size = {"double": 8, "int": 4, "uint": 4, "float": 4, "short": 2, "ushort": 2, "uchar": 1}
    for line in ply[:end].decode("ascii").split("\n"):
        if line.startswith("property "):
            _, t, nm = line.split(" ")[:3]
            props[nm] = (off, t)
            off += size.get(t, 1)
    return end, off, props


def _plant_vertex_numbers(ply):
    """x and f_rest_0 of vertex i become i (neither enters the importance): x travels into the converted row, f_rest_0 into the SH row."""
    ply = bytearray(ply)
    start, row, props = _header(bytes(ply))
    n = (len(ply) - start) // row
    body = np.frombuffer(bytes(ply[start:start + n * row]), np.uint8).reshape(n, row).copy()
    ids = np.arange(n, dtype="<f4").view(np.uint8).reshape(n, 4)
    for nm in ("x", "f_rest_0"):
        assert props[nm][1] == "float"
        body[:, props[nm][0]:props[nm][0] + 4] = ids
    ply[start:start + n * row] = body.tobytes()
    return bytes(ply), n


def _check_order(ply, n, rest=None):
    conv = oracle.ply_to_splat(ply).reshape(-1, 32)
    vertex = conv[:, 0:4].copy().view("<f4").reshape(-1).astype(np.int64)      # which input vertex the oracle placed at j
    assert sorted(vertex.tolist()) == list(range(n))
    sh, d = capi.ply_sh(ply, 3)
    assert d == 3 and sh.shape == (n, 48)
    assert np.array_equal(sh[:, 1].astype(np.int64), vertex)                   # red, k = 1 is f_rest_0
    if rest is not None:
        want = rest[vertex]
        assert np.array_equal(sh.reshape(n, 3, 16)[:, :, 1:].reshape(n, 45)[:, 1:], want[:, 1:])
    for degree, K in ((1, 4), (2, 9)):                                          # a lower degree: the first K of every channel
        low, dl = capi.ply_sh(ply, degree)
        assert dl == degree and np.array_equal(low.reshape(n, 3, K), sh.reshape(n, 3, 16)[:, :, :K])


def test_row_order_on_the_tie_heavy_golden():
    ply, n = _plant_vertex_numbers(bytes(load_case("ply_ties96")["ply"]))
    _check_order(ply, n)


def test_row_order_on_a_synthetic_ply_with_random_f_rest():
    rows = synth.make_splat_rows(5000, seed=77, order_by_importance=False)
    rest = np.random.default_rng(8).standard_normal((5000, 45)).astype(np.float32)
    ply, n = _plant_vertex_numbers(synth.rows_to_inria_ply(rows, rest))
    _check_order(ply, n, rest)


# ---------------------------------------------------------------- 5. header handling

def _ply_with_rest(n_rest, names=None, types=None, n=7, seed=3):
    g = np.random.default_rng(seed)
    names = names or ["f_rest_%d" % i for i in range(n_rest)]
    types = types or ["float"] * len(names)
    props = [("x", "float"), ("y", "float"), ("z", "float"), ("f_dc_0", "float"), ("f_dc_1", "float"), ("f_dc_2", "float")] + \
            list(zip(names, types)) + [(p, "float") for p in ("opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3")]
    np_t = {"float": "<f4", "double": "<f8", "short": "<i2"}
    dt = np.dtype([(nm, np_t[t]) for nm, t in props])
    body = np.zeros(n, dt)
    for nm, t in props:
        body[nm] = g.integers(-300, 300, n) if t == "short" else g.standard_normal(n)
    body["scale_0"] = -np.arange(n)                                            # descending importance in file order: identity order
    body["scale_1"] = body["scale_2"] = 0; body["opacity"] = 0; body["rot_0"] = 1
    hdr = "ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % n + "".join("property %s %s\n" % (t, nm) for nm, t in props) + "end_header\n"
    return hdr.encode("ascii") + body.tobytes(), body


@pytest.mark.parametrize("n_rest,degree", [(0, 0), (9, 1), (24, 2), (45, 3)])
def test_degree_follows_from_the_f_rest_count(n_rest, degree):
    ply, body = _ply_with_rest(n_rest)
    sh, d = capi.ply_sh(ply, 3)
    K = (degree + 1) ** 2
    assert d == degree and sh.shape == (7, 3 * K)
    per = n_rest // 3
    for c in range(3):
        assert np.array_equal(sh.reshape(7, 3, K)[:, c, 0], body["f_dc_%d" % c].astype(np.float32))
        for k in range(1, K):
            assert np.array_equal(sh.reshape(7, 3, K)[:, c, k], body["f_rest_%d" % (c * per + k - 1)].astype(np.float32))
    assert capi.ply_to_splat(ply).size == 7 * 32                               # the converter is unaffected


def test_odd_counts_and_gaps_mean_no_sh():
    for ply in (_ply_with_rest(10)[0],
                _ply_with_rest(9, names=["f_rest_%d" % i for i in (0, 1, 2, 3, 4, 5, 6, 7, 9)])[0]):
        sh, d = capi.ply_sh(ply, 3)
        assert d == -1 and sh.size == 0
        assert capi.ply_to_splat(ply).size == 7 * 32
    sh, d = capi.ply_sh(bytes(load_case("ply_color_only")["ply"]), 3)          # no f_dc_*: red/green/blue
    assert d == -1 and sh.size == 0


@pytest.mark.parametrize("t", ["double", "short"])
def test_f_rest_of_other_declared_types(t):
    ply, body = _ply_with_rest(9, types=[t] * 9)
    sh, d = capi.ply_sh(ply, 1)
    assert d == 1
    for c in range(3):
        for k in range(1, 4):
            assert np.array_equal(sh.reshape(7, 3, 4)[:, c, k], body["f_rest_%d" % (c * 3 + k - 1)].astype(np.float32))


# ---------------------------------------------------------------- 6. the camera

def _rot(ax, deg):
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    m = np.eye(4)
    i, j = [(1, 2), (0, 2), (0, 1)][ax]
    m[i, i], m[i, j], m[j, i], m[j, j] = c, -s, s, c
    return m


def test_camera_in_object_against_numpy_inverse():
    g = np.random.default_rng(12)
    shear = np.eye(4); shear[0, 1], shear[1, 2], shear[0, 2] = 0.7, -0.4, 0.25
    for kind in ("rigid", "scaled", "sheared"):
        for _ in range(20):
            m = _rot(0, g.uniform(-180, 180)) @ _rot(1, g.uniform(-180, 180)) @ _rot(2, g.uniform(-180, 180))
            if kind != "rigid":
                m = m @ np.diag([g.uniform(0.2, 5), g.uniform(0.2, 5), g.uniform(0.2, 5), 1.0])
            if kind == "sheared":
                m = m @ shear
            m[:3, 3] = g.standard_normal(3) * 10
            mv32 = m.T.reshape(-1).astype(np.float32)                          # column-major f32 uniforms
            got = capi.camera_in_object(mv32)
            want = np.linalg.inv(mv32.astype(np.float64).reshape(4, 4).T)[:3, 3]
            assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), (kind, got, want)
    cam = synth.index_html_camera(320, 180, yaw_deg=20.0, capi=capi)
    got = capi.camera_in_object(cam["gs_mv"])
    want = np.linalg.inv(np.asarray(cam["gs_mv"], np.float32).astype(np.float64).reshape(4, 4).T)[:3, 3]
    assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


def test_singular_model_view_is_reported():
    m = np.eye(4); m[2, 2] = 0.0
    with pytest.raises(capi.GsError) as ei:
        capi.camera_in_object(m.T.reshape(-1))
    assert ei.value.code == capi.E_BADARG
    with pytest.raises(capi.GsError):
        capi.camera_in_object(np.zeros(16))
