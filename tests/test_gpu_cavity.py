"""pf_cavity_fwd on a real MI355X (through geometry.cavity_scan and through the C ABI) against the numpy oracle (cavity_oracle.py) on
the cases of cavity_cases.py: the lattice cases against the float64 oracle, the generic ones against the fp32-emulating oracle.

Tolerances.  Every integer output (occupied, buried, label, n_found, size, lining) has to be EQUAL: on the lattice every quantity a
comparison sees is exact in fp32, elsewhere the oracle performs the kernel's fp32 operations in the kernel's order.  center and
mean_buried: 2 fp32 ulp of the tensor's largest magnitude -- derived, the rule of tests/test_gpu_guide.py: both sides accumulate the
same fp32 coordinates (or integers) in double and round once.  The conditions the cases must meet are asserted on the CPU in
tests/test_cavity_cpu.py."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(__file__))
from pepflowww_amd import _capi, geometry  # noqa: E402
import cavity_cases as CC  # noqa: E402
import cavity_oracle as CO  # noqa: E402
import gpu_util as G  # noqa: E402

INT_KEYS = ("occupied", "buried", "label", "n_found", "size", "lining")


@functools.lru_cache(maxsize=None)
def case(name):
    """(the case, its oracle result): computed once and shared; nobody writes to either"""
    c = CC.CASES[name]()
    o = CO.scan(c["pos"], c["mask"], c["aa"], c["radius"], c["origin"], c["dims"], c["h"],
                dtype=np.float64 if c["exact"] else np.float32, **c["params"])
    return c, o


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(G.dev())


def scan(cases, **kw):
    """one call over the cases (same grid and parameters), residues padded with masked ones"""
    n = max(c["pos"].shape[0] for c in cases)
    pos, mask, aa = np.zeros((len(cases), n, 15, 3), np.float32), np.zeros((len(cases), n, 15), bool), np.zeros((len(cases), n), np.int64)
    for b, c in enumerate(cases):
        m = c["pos"].shape[0]
        pos[b, :m], mask[b, :m], aa[b, :m] = c["pos"], c["mask"], c["aa"]
        pos[b, m:] = c["pos"][c["mask"]].mean(0) if c["mask"].any() else 1.0           # masked padding in the middle of the atoms
    c0 = cases[0]
    out = geometry.cavity_scan(cu(pos), cu(mask), cu(aa), cu(np.stack([c["origin"] for c in cases])), c0["dims"], h=c0["h"],
                               radius=cu(c0["radius"]), **{**c0["params"], **kw})
    G.sync()
    return {k: v.cpu().numpy() for k, v in out.items()}


def two_ulp(got, ref64, what):
    """|kernel - float64 reference| <= 2 fp32 ulp of the tensor's largest magnitude"""
    got, ref64 = np.asarray(got, np.float64), np.asarray(ref64, np.float64)
    assert got.shape == ref64.shape and np.isfinite(got).all(), what
    tol = 2.0 * float(np.spacing(np.float32(np.abs(ref64).max()))) if ref64.size else 0.0
    d = float(np.abs(got - ref64).max()) if ref64.size else 0.0
    print(f"{what}: |kernel - oracle| = {d:.3e}, 2 ulp = {tol:.3e}")
    assert d <= tol, (what, d, tol)


def compare(got, b, o, n_res, what):
    """structure b of a call's outputs against the oracle result o"""
    assert int(got["status"][0]) == 0, what
    K = got["size"].shape[1]
    assert K == len(o["size"]), what
    for k in INT_KEYS:
        g = got[k][b]
        if k == "lining":
            assert not g[:, n_res:].any(), (what, "padding residues line nothing")
            g = g[:, :n_res]
        print(f"{what}: {k} differs at {int((np.asarray(g) != o[k]).sum())} of {np.asarray(o[k]).size}")
        assert np.array_equal(g, o[k]), (what, k)
    assert CO.same_partition(got["label"][b], o["label"]), what
    two_ulp(got["center"][b], o["center"], what + " center")
    two_ulp(got["mean_buried"][b], o["mean_buried"], what + " mean_buried")
    n = min(o["n_found"], K)
    for k in ("size", "center", "mean_buried", "lining"):
        assert not got[k][b][n:].any(), (what, k, "rows beyond the found cavities are zero")


@pytest.mark.parametrize("name", list(CC.CASES))
def test_case_against_its_oracle(name):
    c, o = case(name)
    got = scan([c])
    assert got["buried"].dtype == np.uint8 and got["label"].dtype == np.int32 and got["occupied"].dtype == bool
    assert got["label"].shape == (1, int(np.prod(c["dims"]))) and got["lining"].shape == (1, len(o["size"]), c["pos"].shape[0])
    compare(got, 0, o, c["pos"].shape[0], name)


def test_batch_of_three_with_an_empty_structure():
    cases = [case(n) for n in CC.BATCH]
    got = scan([c for c, _ in cases])
    for b, (c, o) in enumerate(cases):
        compare(got, b, o, c["pos"].shape[0], f"batch[{b}] = {CC.BATCH[b]}")
    assert got["n_found"].tolist() == [1, 1, 0] and not got["occupied"][2].any() and (got["label"][2] == -1).all()


def test_max_cavities_cut_and_connectivity_through_the_wrapper():
    c, o = case("many")
    got = scan([c], max_cavities=1)
    assert got["n_found"].tolist() == [6] and got["size"].tolist() == [[5]] and (got["label"][0] >= 0).sum() == 5
    got = scan([c], max_cavities=32)
    assert got["size"][0, :7].tolist() == [5, 4, 3, 3, 2, 1, 0] and got["lining"].shape[1] == 32
    c, _ = case("diagonal_6")
    assert scan([c], connectivity=26)["size"][0, :2].tolist() == [16, 0]


@pytest.mark.parametrize("name", ["serpentine", "generic_150"])
def test_second_call_gives_the_same_bits(name):
    c, _ = case(name)
    a, b = scan([c]), scan([c])
    for k in a:
        assert np.array_equal(a[k].view(np.uint8) if a[k].dtype == np.float32 else a[k], b[k].view(np.uint8) if b[k].dtype == np.float32 else b[k]), k


def _raw_call(c, pad, sentinel):
    """pf_cavity_fwd through the C ABI with `pad` sentinel elements behind every output and behind the scratch"""
    lib = _capi.load()
    dev = G.dev()
    N, (nx, ny, nz), K = c["pos"].shape[0], c["dims"], 4
    Gp = nx * ny * nz
    p = {**CO.DEFAULTS, **c["params"]}
    ins = {"pos": cu(c["pos"]), "atom_mask": cu(c["mask"].astype(np.uint8)), "aa": cu(c["aa"]), "radius": cu(c["radius"]),
           "origin": cu(c["origin"])}
    shapes = {"occupied": (torch.uint8, Gp), "buried": (torch.uint8, Gp), "label": (torch.int32, Gp), "n_found": (torch.int32, 1),
              "size": (torch.int32, K), "center": (torch.float32, 3 * K), "mean_buried": (torch.float32, K),
              "lining": (torch.uint8, K * N), "status": (torch.int32, 1), "work": (torch.uint8, lib.pf_cavity_work_bytes(nx, ny, nz))}
    outs = {k: torch.full((n + pad,), sentinel, dtype=dt, device=dev) for k, (dt, n) in shapes.items()}
    a = _capi.CavityArgs()
    for k, t in {**ins, **outs}.items():
        setattr(a, k, t.data_ptr())
    a.B, a.N, a.n_atoms, a.nx, a.ny, a.nz = 1, N, 15, nx, ny, nz
    a.n_axis, a.n_diag = CO.steps(c["h"], p["max_ray"])
    a.min_buried, a.connectivity, a.min_points, a.max_cavities = p["min_buried"], p["connectivity"], p["min_points"], K
    a.h, a.probe, a.r_lining = c["h"], p["probe"], p["r_lining"]
    _capi.check(lib.pf_cavity_fwd(C.byref(a), _capi.stream_ptr()), "pf_cavity_fwd")
    G.sync()
    return {k: t.cpu() for k, t in outs.items()}, {k: n for k, (_, n) in shapes.items()}


def test_nothing_is_written_beyond_the_outputs_or_the_scratch():
    for name in ("shell", "generic_40"):
        c, o = case(name)
        outs, sizes = _raw_call(c, 64, 77)
        for k, t in outs.items():
            assert (t[sizes[k]:] == 77).all(), (name, k)
        assert int(outs["status"][0]) == 0 and int(outs["n_found"][0]) == o["n_found"]
        assert np.array_equal(outs["label"][:sizes["label"]].numpy(), o["label"]), name
        assert np.array_equal(outs["size"][:4].numpy(), o["size"][:4]), name


def test_call_inside_a_captured_graph_replayed_twice():
    c, o = case("groove")
    dev = G.dev()
    pos, mask, aa = cu(c["pos"][None]), cu(c["mask"][None]), cu(c["aa"][None])
    origin, radius = cu(c["origin"][None]), cu(c["radius"])
    call = lambda: geometry.cavity_scan(pos, mask, aa, origin, c["dims"], h=c["h"], radius=radius, **c["params"])  # noqa: E731
    eager = {k: v.cpu() for k, v in call().items()}
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with _capi.capture_guard(), torch.cuda.graph(g, stream=s):
            out = call()                                    # no host read inside: the status word is checked after the replay
    torch.cuda.synchronize()
    for rep in range(2):
        for v in out.values():
            v.view(torch.uint8).fill_(9)                    # what a replay does not write would stay
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        geometry.cavity_check(out["status"])
        for k, v in out.items():
            assert torch.equal(v.cpu(), eager[k]), (rep, k)
    assert np.array_equal(out["label"][0].cpu().numpy(), o["label"]) and dev.type == "cuda"
