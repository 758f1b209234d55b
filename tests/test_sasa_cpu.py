"""CPU checks of the solvent-accessible surface: the sphere-point and radius tables, the numpy float64 oracle (sasa_oracle.py) against
exact answers and against the two-sphere cap formula, the argument checks of geometry.sasa and metrics.interface_area, the C ABI's
bounds."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import sasa_oracle as SO  # noqa: E402
from pepflowww_amd import _capi, geometry, metrics  # noqa: E402
from pepflowww_amd.preprocess import _tables, residue_type  # noqa: E402

RADIUS = geometry.sasa_radius_table().numpy()
GLY, CYS = residue_type("GLY"), residue_type("CYS")
C_RAD, O_RAD, PROBE = 1.7, 1.52, 1.4


def atoms(*specs, n_res=None):
    """specs: (residue, slot, xyz) of glycines (slot 0 N, 1 CA, 2 C, 3 O) -> pos [N,15,3] fp32, mask [N,15], aa [N]"""
    n = 1 + max(r for r, _, _ in specs) if n_res is None else n_res
    pos, mask = np.zeros((n, 15, 3), np.float32), np.zeros((n, 15), bool)
    for r, s, x in specs:
        pos[r, s] = x
        mask[r, s] = True
    return pos, mask, np.full(n, GLY, np.int64)


def points(P):
    return geometry.sphere_points(P).numpy()


def test_sphere_points():
    """Unit norms to 2^-23, the same table on every call, and P = 1: y = 0, r = 1, phi = 0 gives (1, 0, 0)."""
    for P in (1, 2, 64, 92, 960, 1024):
        u = geometry.sphere_points(P)
        assert u.shape == (P, 3) and u.dtype == torch.float32 and not u.is_cuda
        assert (np.abs(np.linalg.norm(u.numpy().astype(np.float64), axis=1) - 1.0) <= 2.0 ** -23).all(), P
        assert torch.equal(u, geometry.sphere_points(P))
    assert geometry.sphere_points(1).tolist() == [[1.0, 0.0, 0.0]]
    k = np.arange(92, dtype=np.float64)
    y = (2 * k + 1) / 92 - 1
    phi = k * np.pi * (3 - np.sqrt(5.0))
    want = np.stack([np.sqrt(1 - y * y) * np.cos(phi), y, np.sqrt(1 - y * y) * np.sin(phi)], 1)
    assert np.abs(points(92) - want).max() <= 2.0 ** -24
    for bad in (0, 1025, -3, 2.5, None, True):
        with pytest.raises(ValueError):
            geometry.sphere_points(bad)


def test_radius_table_against_the_atom_names():
    assert RADIUS.shape == (21, 15) and RADIUS.dtype == np.float32
    assert np.array_equal(RADIUS[:, :14], geometry.vdw_radius_table().numpy())
    assert (RADIUS[:, 14] == np.float32(1.52)).all()
    names = _tables()["atom_names"]
    for t in range(20):
        assert names[t][14] == "OXT"
        for s in range(14):
            want = geometry.VDW_RADIUS[names[t][s][0]] if names[t][s] else 0.0
            assert RADIUS[t, s] == np.float32(want), (t, s)
    assert np.array_equal(RADIUS[20], np.array([1.55, 1.7, 1.7, 1.52] + [0.0] * 10 + [1.52], np.float32))
    assert RADIUS[CYS, 5] == np.float32(1.8) and RADIUS.max() == np.float32(1.8)
    apolar = metrics.apolar_table().numpy()
    assert apolar.shape == (21, 15) and apolar[CYS, 5] and apolar[GLY, :4].tolist() == [False, True, True, False]
    assert not apolar[:, 14].any() and np.array_equal(apolar, np.isin(RADIUS, np.float32([1.7, 1.8])))


@pytest.mark.parametrize("P", [1, 64, 92, 960])
def test_oracle_exact_answers(P):
    u = points(P)
    sphere = lambda r: 4 * np.pi * float(np.float32(r) + np.float32(PROBE)) ** 2  # noqa: E731
    # an isolated atom
    o = SO.sasa(*atoms((0, 1, [3.0, -2.0, 7.0])), RADIUS, u)
    assert o["count"][0, 1] == P and o["count"].sum() == P and o["marginal"].sum() == 0
    assert abs(o["sasa_atom"][0, 1] - sphere(C_RAD)) <= 1e-12 * sphere(C_RAD) and abs(o["sasa_total"] - sphere(C_RAD)) <= 1e-9
    assert "count_own" not in o
    # an oxygen inside a coincident carbon: the larger buries the smaller
    o = SO.sasa(*atoms((0, 1, [1.0, 1.0, 1.0]), (1, 3, [1.0, 1.0, 1.0])), RADIUS, u)
    assert o["count"][0, 1] == P and o["count"][1, 3] == 0 and o["marginal"].sum() == 0
    # two atoms beyond R_a + R_b = 3.1 + 2.92, of one residue and of two
    for spec in (((0, 1, [0.0, 0.0, 0.0]), (0, 3, [6.03, 0.0, 0.0])), ((0, 1, [0.0, 0.0, 0.0]), (1, 3, [0.0, 6.03, 0.0]))):
        o = SO.sasa(*atoms(*spec), RADIUS, u)
        assert o["count"].sum() == 2 * P and o["marginal"].sum() == 0
    # closer than that each loses points (P = 1: the one point (1, 0, 0) of the atom on the left faces its partner), the same
    # residue counts, and a masked partner buries nothing
    for spec in (((0, 1, [0.0, 0.0, 0.0]), (0, 3, [3.0, 0.0, 0.0])), ((0, 1, [0.0, 0.0, 0.0]), (1, 3, [3.0, 0.0, 0.0]))):
        pos, mask, aa = atoms(*spec)
        o = SO.sasa(pos, mask, aa, RADIUS, u)
        assert o["count"][0, 1] < P and (P == 1 or 0 < o["count"][0, 1]) and (P == 1 or o["count"][spec[1][0], 3] < P)
        mask[spec[1][0], 3] = False
        o = SO.sasa(pos, mask, aa, RADIUS, u)
        assert o["count"][0, 1] == P and o["count"].sum() == P
    # a slot without a radius (glycine has no slot 4) is no atom
    pos, mask, aa = atoms((0, 1, [0.0, 0.0, 0.0]), (0, 4, [1.0, 0.0, 0.0]))
    assert SO.sasa(pos, mask, aa, RADIUS, u)["count"].sum() == P


@pytest.mark.parametrize("P", [64, 960])
def test_oracle_group_and_query(P):
    u = points(P)
    # residue 2 alone in its group next to two residues of the other
    pos, mask, aa = atoms((0, 1, [0.0, 0.0, 0.0]), (1, 1, [3.5, 0.0, 0.0]), (2, 1, [1.7, 2.5, 0.0]), (2, 3, [30.0, 0.0, 0.0]))
    group = np.array([0, 0, 1])
    o = SO.sasa(pos, mask, aa, RADIUS, u, group=group)
    plain = SO.sasa(pos, mask, aa, RADIUS, u)
    assert np.array_equal(o["count"], plain["count"]) and (o["count_own"] >= o["count"]).all()
    assert o["count_own"][2, 1] == P and o["count"][2, 1] < P and o["count_own"][2, 3] == P
    assert o["count"][0, 1] < o["count_own"][0, 1] < P                      # residue 1 buries part of it within its group
    alone = SO.sasa(pos[:2], mask[:2], aa[:2], RADIUS, u)
    assert np.array_equal(alone["count"], o["count_own"][:2])               # a group on its own IS that group without the rest
    assert abs(o["sasa_total_own"] - o["sasa_atom_own"].sum()) <= 1e-9 and o["sasa_total_own"] > o["sasa_total"]
    # query: the others are partners still, but not evaluated
    q = SO.sasa(pos, mask, aa, RADIUS, u, query=np.array([0, 0, 1]), group=group)
    assert np.array_equal(q["count"][2], o["count"][2]) and np.array_equal(q["count_own"][2], o["count_own"][2])
    assert q["count"][0, 1] == q["count"][1, 1] == q["count_own"][0, 1] == -1 and q["count"][0, 0] == 0
    assert q["sasa_residue"][:2].sum() == 0 and abs(q["sasa_total"] - o["sasa_residue"][2]) <= 1e-9


@pytest.mark.parametrize("P", [64, 92, 960])
def test_oracle_against_the_two_sphere_cap(P):
    """A carbon and an oxygen d apart along x, y (the spiral's axis) or z, d = 0.3 .. 6.3 A in 61 steps: the share of a's sphere inside b's is the cap h / 2 R_a, h = R_a -
    (d^2 + R_a^2 - R_b^2) / 2d, clipped to [0, 1].  The oracle's accessible share must agree within 0.5 / sqrt(P), the quadrature's
    bound (a ring of the spiral holds about sqrt(P) points, and the cap's rim cuts about one ring); the worst seen is 0.34 / sqrt(P), at
    P = 64 along x.  It checks the oracle, not the kernel."""
    u = points(P)
    Ra, Rb = float(np.float32(C_RAD) + np.float32(PROBE)), float(np.float32(O_RAD) + np.float32(PROBE))
    worst = 0.0
    for d, axis in ((d, axis) for d in np.linspace(0.3, 6.3, 61) for axis in range(3)):
        o = SO.sasa(*atoms((0, 1, [0.0, 0.0, 0.0]), (1, 3, np.eye(3)[axis] * d)), RADIUS, u)
        for (n, s), R, Ro in (((0, 1), Ra, Rb), ((1, 3), Rb, Ra)):
            h = R - (d * d + R * R - Ro * Ro) / (2 * d)
            want = 1.0 - min(max(h / (2 * R), 0.0), 1.0)
            worst = max(worst, abs(o["count"][n, s] / P - want))
    print(f"P = {P}: worst deviation {worst * np.sqrt(P):.3f} / sqrt(P)")
    assert worst <= 0.5 / np.sqrt(P), worst * np.sqrt(P)


def test_oracle_marginal_points():
    """A partner whose surface passes within eps of a point makes that point marginal, on either side of it."""
    u = points(92)
    Ra, Rb = float(np.float32(C_RAD) + np.float32(PROBE)), float(np.float32(O_RAD) + np.float32(PROBE))
    eps = SO.margin_eps(RADIUS, PROBE)
    assert abs(eps - 32 * 2.0 ** -23 * 2 * (1.8 + 1.4)) < 1e-9
    k = 17
    for off, buried in ((0.25 * eps, 1), (-0.25 * eps, 0), (1e-3, 1), (-1e-3, 0)):
        # the oxygen on the ray through point k, its surface `off` beyond the point
        b = u[k].astype(np.float64) * (Ra + Rb - off)
        o = SO.sasa(*atoms((0, 1, [0.0, 0.0, 0.0]), (1, 3, b)), RADIUS, u)
        assert o["marginal"][0, 1] == (1 if abs(off) < eps else 0), off
        assert o["count"][0, 1] == 92 - buried or abs(off) < eps


def test_wrapper_argument_checks():
    pos = torch.zeros(2, 5, 15, 3)
    ok = dict(atom_mask=torch.ones(2, 5, 15, dtype=torch.bool), aa=torch.zeros(2, 5, dtype=torch.int64))
    with pytest.raises(ValueError):
        geometry.sasa(torch.zeros(2, 5, 4, 3), torch.ones(2, 5, 4, dtype=torch.bool), ok["aa"])
    with pytest.raises(ValueError):
        geometry.sasa(pos, ok["atom_mask"][:, :, :14], ok["aa"])
    with pytest.raises(ValueError):
        geometry.sasa(pos, **ok, query=torch.ones(2, 4, dtype=torch.bool))
    with pytest.raises(ValueError):
        geometry.sasa(pos, **ok, group=torch.ones(5, dtype=torch.bool))
    with pytest.raises(ValueError):
        geometry.sasa(torch.zeros(1, 513, 15, 3), torch.ones(1, 513, 15, dtype=torch.bool), torch.zeros(1, 513, dtype=torch.int64))
    for bad in (0, 1025, 92.0):
        with pytest.raises(ValueError):
            geometry.sasa(pos, **ok, n_points=bad)
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            geometry.sasa(pos, **ok, probe_radius=bad)
    with pytest.raises(_capi.PepflowHipError):              # CPU tensors: no fall-back
        geometry.sasa(pos, **ok)
    with pytest.raises(ValueError):
        metrics.interface_area({}, {}, backbone="atoms")
    with pytest.raises(ValueError):
        metrics.interface_area({}, {}, n_points=0)
    with pytest.raises(ValueError):
        metrics.interface_area({}, {}, probe_radius=-1.0)


def test_c_abi_bounds():
    lib = _capi.load()
    assert lib.pf_abi_version() == _capi.ABI_VERSION
    assert "pf_sasa_fwd" in _capi.EXPORTED_SYMBOLS
    assert lib.pf_sasa_fwd(None, None) == -1
    a = _capi.SasaArgs()
    assert lib.pf_sasa_fwd(C.byref(a), None) == -1
    # every pointer set (never dereferenced: the checks come first) and one bad scalar at a time
    buf = (C.c_char * 64)()
    good = dict(B=1, N=4, n_atoms=15, n_points=92, probe_radius=1.4)

    def filled(**kw):
        a = _capi.SasaArgs()
        for name, typ in _capi.SasaArgs._fields_:
            if typ is C.c_void_p and name not in ("query", "group", "count_own", "sasa_atom_own", "sasa_residue_own", "sasa_total_own"):
                setattr(a, name, C.addressof(buf))
        for k, v in {**good, **kw}.items():
            setattr(a, k, v)
        return a

    for kw in (dict(n_atoms=13), dict(n_points=0), dict(n_points=1025), dict(probe_radius=-0.5), dict(probe_radius=float("nan")),
               dict(B=-1), dict(N=-1), dict(count_own=C.addressof(buf))):
        assert lib.pf_sasa_fwd(C.byref(filled(**kw)), None) == -1, kw
    assert lib.pf_sasa_fwd(C.byref(filled(N=513)), None) == -2
    assert lib.pf_sasa_fwd(C.byref(filled(B=65536)), None) == -2
    assert lib.pf_sasa_fwd(C.byref(filled(B=0)), None) == 0              # an empty batch: nothing is launched
