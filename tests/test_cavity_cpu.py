"""CPU checks of the de novo design entry: the cavity cases meet their conditions (the lattice is exact in fp32, each constructed
answer, the float64 and the fp32-emulating oracle agree on every lattice case, the oracle's index box against its brute-force form),
the ctypes struct against the header, the entry points' argument checks, geometry.cavity_grid / cavity_scan's argument checks, and
design.make_design_batch: the round trip against preprocess_structure, the selection rule and the argument errors."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import cavity_cases as CC  # noqa: E402
import cavity_oracle as CO  # noqa: E402
from test_lddt_cpu import HEADER, header_fields  # noqa: E402
from pepflowww_amd import _capi, build, design, geometry, io, preprocess, synth  # noqa: E402


def oracle(c, dtype, **kw):
    return CO.scan(c["pos"], c["mask"], c["aa"], c["radius"], c["origin"], c["dims"], c["h"], dtype=dtype, **kw, **c["params"])


@pytest.fixture(scope="module")
def lattice():
    return {name: (c, oracle(c, np.float64)) for name, c in ((n, mk()) for n, mk in CC.LATTICE.items())}


# ---- the cases -----------------------------------------------------------------------------------------------------------------------

def test_lattice_cases_are_exact_in_fp32(lattice):
    for name, (c, _) in lattice.items():
        for v in (c["pos"][c["mask"]], c["origin"], c["radius"], np.float32(c["h"]), np.float32(c["params"]["probe"]),
                  np.float32(c["params"]["r_lining"])):
            v = np.asarray(v, np.float64)
            assert (v * 8 == np.round(v * 8)).all() and (np.abs(v) < 64).all(), name
        assert c["h"] in (1.0, 0.5)
        far = max(np.abs(np.float64(c["origin"][k]) + (c["dims"][k] - 1) * c["h"]) for k in range(3))
        # a difference is a multiple of 1/8 below 128, its square a multiple of 1/64 below 2^14, the sum of three below 2^16:
        # 6 + 16 = 22 bits, inside fp32's 24
        assert far < 64, name


def test_float64_and_fp32_oracles_agree_on_the_lattice(lattice):
    for name, (c, o64) in lattice.items():
        o32 = oracle(c, np.float32)
        for k in ("occupied", "buried", "label", "size", "lining"):
            assert np.array_equal(o64[k], o32[k]), (name, k)
        assert o64["n_found"] == o32["n_found"] and np.array_equal(o64["center"], o32["center"]), name
        assert np.array_equal(o64["mean_buried"], o32["mean_buried"]), name


def test_constructed_answers(lattice):
    for name, (c, o) in lattice.items():
        ans = c["answer"]
        assert o["n_found"] == ans["n_found"], name
        n = len(ans.get("size", ()))
        assert o["size"][:n].tolist() == ans.get("size", []) and (o["size"][max(n, min(o["n_found"], len(o["size"]))):] == 0).all(), name
        if "center" in ans:
            assert np.array_equal(o["center"][:n], np.asarray(ans["center"])), name
        if "mean_buried" in ans:
            assert o["mean_buried"][:n].tolist() == ans["mean_buried"], name


def test_cases_cover_what_they_are_for(lattice):
    c, o = lattice["shell"]
    assert (o["buried"][o["label"] == 0] == 7).all() and o["lining"][0].sum() > 0 and not o["lining"][0, :3].any()    # masked residues
    assert o["occupied"].sum() == c["mask"].sum()                                       # h = 1: an atom occupies its own point only
    assert lattice["shell_half"][1]["occupied"].sum() > 10 * c["mask"].sum() and lattice["shell_half"][1]["size"][0] > 8 * 315 * 0.8
    c, o = lattice["groove"]
    member = (o["label"] == 0).reshape(c["dims"])
    assert member[3:10, 2:7, 4].all() and not member[:, :, 13:].any() and o["buried"][o["label"] == 0].max() == 6    # the floor; open
    assert lattice["diagonal_6"][1]["size"][:2].tolist() == [8, 8] and lattice["diagonal_26"][1]["size"][0] == 16
    c, o = lattice["serpentine"]
    blocks = np.unique(np.nonzero(o["label"] == 0)[0] // 256)
    assert len(blocks) >= 12                                                            # one component across a dozen workgroups
    c, o = lattice["many"]
    assert c["pos"].shape[0] > 512 and o["n_found"] > c["params"]["max_cavities"] and (o["label"] >= 0).sum() == 12
    c, o = lattice["empty"]
    assert not o["occupied"].any() and not o["buried"].any() and (o["label"] == -1).all()
    for dims in ((13, 9, 17), (33, 20, 7), (3, 3, 3)):
        assert any(c["dims"] == dims for c, _ in lattice.values())
    assert all(lattice[n][0]["dims"] == lattice[CC.BATCH[0]][0]["dims"] for n in CC.BATCH)
    assert len({lattice[n][0]["pos"].shape[0] for n in CC.BATCH}) == 3


def test_oracle_index_box_is_the_brute_force_and_partitions_compare():
    for c in (CC.shell_half(), CC.generic(40, 11)):
        dt = np.float64 if c["exact"] else np.float32
        a, b = oracle(c, dt), oracle(c, dt, brute=True)
        assert np.array_equal(a["occupied"], b["occupied"]) and np.array_equal(a["label"], b["label"])
    assert CO.same_partition([0, 0, 1, -1], [1, 1, 0, -1]) and not CO.same_partition([0, 0, 1, -1], [0, 1, 1, -1])
    assert not CO.same_partition([0, 0, -1], [0, 0, 0]) and not CO.same_partition([0, 1], [0, 0])
    assert CO.steps(1.0, 12.0) == (12, 6) and CO.steps(0.5, 12.0) == (24, 13)


def test_generic_cases_have_cavities_and_unrounded_coordinates():
    for name, mk in CC.GENERIC.items():
        c = mk()
        o = oracle(c, np.float32)
        assert o["n_found"] >= 2 and o["lining"][0].sum() >= 5, name
        assert (c["pos"][c["mask"]] * 8 != np.round(c["pos"][c["mask"]] * 8)).mean() > 0.9, name


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------

def test_struct_layout_header_order_and_additive_abi():
    assert [(n, t) for n, t in _capi.CavityArgs._fields_] == header_fields("pf_cavity_args")
    assert _capi.CavityArgs.r_lining.offset + 4 <= C.sizeof(_capi.CavityArgs) and C.sizeof(_capi.CavityArgs) % 8 == 0
    text = open(HEADER).read()
    assert "#define PF_ABI_VERSION 65" in text and _capi.ABI_VERSION == 65
    assert "#define PF_CAVITY_MAX_N 4096" in text and geometry.CAVITY_MAX_N == 4096
    assert "#define PF_CAVITY_MAX_POINTS 2097152" in text and geometry.CAVITY_MAX_POINTS == 128 ** 3 == 2097152
    assert "#define PF_CAVITY_MAX_OUT 32" in text and geometry.CAVITY_MAX_OUT == 32
    assert text.index("} pf_sasa_args;") < text.index("} pf_cavity_args;") < text.index("int pf_cavity_fwd(") < \
        text.index("int pf_cavity_work_bytes(") < text.index("} pf_torsions_args;")
    i = build.SOURCES.index("cavity.hip")
    assert build.SOURCES[i - 1] == "sasa.hip" and build.SOURCES[i + 1] == "torsions.hip"
    k = _capi.EXPORTED_SYMBOLS.index("pf_sasa_fwd")
    assert _capi.EXPORTED_SYMBOLS[k + 1:k + 4] == ("pf_cavity_fwd", "pf_cavity_work_bytes", "pf_torsions_fwd")
    assert geometry.CAVITY_DEFAULTS == CO.DEFAULTS


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """every pointer is a host buffer here: a call that got as far as a launch would not return an argument error"""
    lib = _capi.load()
    assert lib.pf_cavity_fwd(None, None) == -1
    assert lib.pf_cavity_fwd(C.byref(_capi.CavityArgs()), None) == -1
    buf = (C.c_char * 64)()
    good = dict(B=1, N=4, n_atoms=15, nx=8, ny=8, nz=8, n_axis=12, n_diag=6, min_buried=5, connectivity=6, min_points=8,
                max_cavities=8, h=1.0, probe=1.4, r_lining=4.5)

    def args(**kw):
        a = _capi.CavityArgs()
        for name, typ in _capi.CavityArgs._fields_:
            if typ is C.c_void_p:
                setattr(a, name, C.addressof(buf))
        for k, v in {**good, **kw}.items():
            setattr(a, k, v)
        return a

    for name, typ in _capi.CavityArgs._fields_:
        if typ is C.c_void_p:
            assert lib.pf_cavity_fwd(C.byref(args(**{name: None})), None) == -1, name
    for bad in (dict(B=-1), dict(N=-1), dict(n_atoms=13), dict(nx=0), dict(ny=-1), dict(nz=0), dict(n_axis=-1), dict(n_diag=-1),
                dict(min_buried=0), dict(min_buried=8), dict(connectivity=18), dict(min_points=0), dict(max_cavities=0),
                dict(max_cavities=33), dict(h=0.0), dict(h=float("nan")), dict(h=float("inf")), dict(probe=-1.0),
                dict(probe=float("nan")), dict(r_lining=-1.0), dict(r_lining=float("inf"))):
        assert lib.pf_cavity_fwd(C.byref(args(**bad)), None) == -1, bad
    for big in (dict(N=4097), dict(B=65536), dict(nx=129, ny=128, nz=128), dict(nx=65536, ny=65536, nz=1)):
        assert lib.pf_cavity_fwd(C.byref(args(**big)), None) == -2, big
    assert lib.pf_cavity_fwd(C.byref(args(B=0)), None) == 0                             # an empty batch: nothing is launched
    assert lib.pf_cavity_work_bytes(8, 8, 8) == 4 * ((1 + 64 + 32 * 24 + 3) // 4 * 4 + 3 * 512)
    assert lib.pf_cavity_work_bytes(128, 128, 128) == 4 * ((1 + 64 + 32 * 384 + 3) // 4 * 4 + 3 * 128 ** 3)
    for bad in ((0, 8, 8), (8, -1, 8), (129, 128, 128), (65536, 65536, 2)):
        assert lib.pf_cavity_work_bytes(*bad) == -1, bad


def test_wrapper_argument_checks():
    pos, mask, aa = torch.zeros(2, 5, 15, 3), torch.ones(2, 5, 15, dtype=torch.bool), torch.zeros(2, 5, dtype=torch.int64)
    origin, dims = torch.zeros(2, 3), (8, 8, 8)
    for bad in (dict(h=0.0), dict(h=-1.0), dict(h=float("nan")), dict(min_buried=0), dict(min_buried=8), dict(min_buried=5.0),
                dict(connectivity=18), dict(min_points=0), dict(max_cavities=0), dict(max_cavities=33), dict(probe=-0.1),
                dict(max_ray=float("nan")), dict(r_lining=-1.0), dict(nonsense=1), dict(radius=torch.zeros(20, 15))):
        with pytest.raises(ValueError):
            geometry.cavity_scan(pos, mask, aa, origin, dims, **bad)
    for bad_dims in ((0, 8, 8), (129, 128, 128), (8, 8), "abc"):
        with pytest.raises(ValueError):
            geometry.cavity_scan(pos, mask, aa, origin, bad_dims)
    with pytest.raises(ValueError):
        geometry.cavity_scan(pos, mask, aa, torch.zeros(3), dims)
    with pytest.raises(ValueError):
        geometry.cavity_scan(pos, mask[:, :, :14], aa, origin, dims)
    with pytest.raises(ValueError):
        geometry.cavity_scan(torch.zeros(1, 4097, 15, 3), torch.ones(1, 4097, 15, dtype=torch.bool), torch.zeros(1, 4097, dtype=torch.int64),
                             torch.zeros(1, 3), dims)
    with pytest.raises(_capi.PepflowHipError):              # CPU tensors: no fall-back
        geometry.cavity_scan(pos, mask, aa, origin, dims)


def test_cavity_grid():
    pos = torch.zeros(2, 2, 15, 3)
    mask = torch.zeros(2, 2, 15, dtype=torch.bool)
    pos[0, 0, 0], pos[0, 1, 3] = torch.tensor([1.2, -3.7, 10.0]), torch.tensor([4.9, 2.0, 11.6])
    mask[0, 0, 0] = mask[0, 1, 3] = True
    pos[0, 1, 5] = 1e6                                      # masked: not part of the box
    origin, dims = geometry.cavity_grid(pos, mask, h=0.5, margin=2.0)
    assert origin.dtype == torch.float32 and origin[0].tolist() == [-1.0, -6.0, 8.0] and origin[1].tolist() == [0.0, 0.0, 0.0]
    assert dims == (17, 21, 13)                             # x: -1.0 .. 7.0, y: -6.0 .. 4.0, z: 8.0 .. 14.0 (13.6 rounded up)
    lo, hi = origin[0].double(), origin[0].double() + (torch.tensor(dims) - 1) * 0.5
    assert (lo <= torch.tensor([1.2, -3.7, 10.0]) - 2.0).all() and (hi >= torch.tensor([4.9, 2.0, 11.6]) + 2.0).all()
    for bad in (dict(h=0.0), dict(margin=-1.0), dict(h=float("inf"))):
        with pytest.raises(ValueError):
            geometry.cavity_grid(pos, mask, **bad)
    with pytest.raises(ValueError):
        geometry.cavity_grid(pos[0], mask[0])


# ---- design.make_design_batch --------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def complex_dir(tmp_path_factory):
    """a synthetic complex of 30 receptor and 9 peptide residues written as pocket.pdb / peptide.pdb, and the receptor alone"""
    d = tmp_path_factory.mktemp("complex")
    c = synth.make_pocket(np.random.Generator(np.random.PCG64(5)), 30, 9)
    c["pos_heavyatom"] = c["pos_heavyatom"] + np.float32([11.0, -7.0, 23.0])       # not centred: the entry has to do that
    t = {k: torch.from_numpy(v) for k, v in c.items()}
    n = t["aa"].shape[0]
    for name, rows, chain in (("pocket.pdb", slice(0, 30), "B"), ("peptide.pdb", slice(30, n), "A")):
        m = rows.stop - rows.start
        io.write_pdb({"aa": t["aa"][rows], "pos_heavyatom": t["pos_heavyatom"][rows], "mask_heavyatom": t["mask_heavyatom"][rows],
                      "chain_nb": torch.zeros(m, dtype=torch.int64), "chain_id": [chain] * m, "resseq": torch.arange(1, m + 1),
                      "icode": [" "] * m}, str(d / name))
    return d


def test_design_batch_round_trip_against_preprocess_structure(complex_dir):
    want = preprocess.preprocess_structure({"id": "x", "pdb_path": str(complex_dir)})
    pep = preprocess.parse_pdb(str(complex_dir / "peptide.pdb"))[0]
    ok = pep["mask_heavyatom"][:, preprocess.CA]
    center = pep["pos_heavyatom"][ok, preprocess.CA].sum(0) / (ok.sum() + 1e-8)
    rec = design.receptor_from_pdb(str(complex_dir / "pocket.pdb"))
    n_rec, n_pep = rec["aa"].shape[0], pep["aa"].shape[0]
    assert n_rec == 30 and n_pep == 9 and rec["torsion_angle"].shape == (30, 5)
    batch, info = design.make_design_batch(rec, n_pep, 3, center=center, radius=1e3)
    L = batch["aa"].shape[1]
    assert L == 40 and L % 8 == 0 and info["context_index"].tolist() == list(range(n_rec)) and info["site"] == "center"
    assert set(batch) == set(want) | {"res_mask"}
    for k, v in want.items():
        if not isinstance(v, torch.Tensor):
            continue
        assert batch[k].shape == (3,) + (L,) + v.shape[1:] and batch[k].dtype == v.dtype, k
        assert torch.equal(batch[k][0], batch[k][1]) and torch.equal(batch[k][0], batch[k][2]), k
        assert torch.equal(batch[k][0, :n_rec], v[:n_rec]), k                           # the receptor rows, entry by entry
    for k in ("res_nb", "chain_nb", "generate_mask"):
        assert torch.equal(batch[k][0, n_rec:n_rec + n_pep], want[k][n_rec:]), k        # the peptide rows' bookkeeping
    assert batch["res_mask"][0].tolist() == [True] * (n_rec + n_pep) + [False] * (L - n_rec - n_pep)
    rows = slice(n_rec, n_rec + n_pep)
    assert (batch["aa"][0, rows] == preprocess.UNK).all() and not batch["pos_heavyatom"][0, rows].any()
    assert batch["mask_heavyatom"][0, rows, :4].all() and not batch["mask_heavyatom"][0, rows, 4:].any()
    assert not batch["torsion_angle"][0, rows].any()
    assert batch["torsion_angle_mask"][0, rows, 0].all() and not batch["torsion_angle_mask"][0, rows, 1:].any()
    assert (batch["aa"][0, n_rec + n_pep:] == io.PAD_AA).all() and not batch["mask_heavyatom"][0, n_rec + n_pep:].any()
    assert torch.equal(info["center"], center) and not info["hotspots"].any() and info["hotspots"].shape == (L,)
    x = batch["pos_heavyatom"][0, :n_rec]
    assert torch.allclose(design.to_receptor_frame(x, info), rec["pos_heavyatom"], atol=1e-5)
    only_b = design.receptor_from_pdb(str(complex_dir / "pocket.pdb"), chains=["B"])
    assert torch.equal(only_b["pos_heavyatom"], rec["pos_heavyatom"])
    with pytest.raises(ValueError):
        design.receptor_from_pdb(str(complex_dir / "pocket.pdb"), chains=["Z"])


def _line_receptor(n=12):
    """CA-only residues on the x axis, 2 A apart, residue i at x = 2 i"""
    pos = torch.zeros(n, 15, 3)
    pos[:, 1, 0] = 2.0 * torch.arange(n)
    mask = torch.zeros(n, 15, dtype=torch.bool)
    mask[:, 1] = True
    return {"chain_id": ["A"] * n, "chain_nb": torch.zeros(n, dtype=torch.int64), "resseq": torch.arange(1, n + 1), "icode": [" "] * n,
            "res_nb": torch.arange(1, n + 1), "aa": torch.zeros(n, dtype=torch.int64), "pos_heavyatom": pos, "mask_heavyatom": mask}


def test_selection_rule_radius_max_context_and_ties():
    rec = _line_receptor()
    _, info = design.make_design_batch(rec, 4, 1, center=[10.0, 0.0, 0.0], radius=4.0)
    assert info["context_index"].tolist() == [3, 4, 5, 6, 7]                            # |x - 10| <= 4, the bound included
    _, info = design.make_design_batch(rec, 4, 1, center=[10.0, 0.0, 0.0], radius=4.0, max_context=2)
    assert info["context_index"].tolist() == [4, 5]                                     # 5 at 0 A; 4 and 6 tie at 2 A: the lower index
    _, info = design.make_design_batch(rec, 4, 1, center=[10.0, 0.0, 0.0], radius=4.0, max_context=4)
    assert info["context_index"].tolist() == [3, 4, 5, 6]                               # receptor order, not order of distance
    batch, info = design.make_design_batch(rec, 4, 2, hotspots=[2, 4], radius=3.0)
    assert info["site"] == "hotspots" and info["center"].tolist() == [6.0, 0.0, 0.0] and info["context_index"].tolist() == [2, 3, 4]
    assert info["hotspots"].tolist() == [True, False, True] + [False] * 5 and batch["aa"].shape == (2, 8)
    assert batch["pos_heavyatom"][0, :3, 1, 0].tolist() == [-2.0, 0.0, 2.0] and batch["chain_nb"][0].tolist() == [1, 1, 1, 0, 0, 0, 0, 0]
    cav = {"center": torch.tensor([1.0, 0.0, 0.0]), "points": torch.tensor([[0.0, 0.0, 0.0], [20.0, 0.0, 0.0]]),
           "lining": torch.tensor([0, 10, 5])}
    _, info = design.make_design_batch(rec, 3, 1, cavity=cav, radius=1.0)                # every member point counts, not the centre
    assert info["context_index"].tolist() == [0, 10] and info["hotspots"][:2].tolist() == [True, True] and info["site"] == "cavity"
    masked = _line_receptor()
    masked["mask_heavyatom"][5] = False
    _, info = design.make_design_batch(masked, 4, 1, center=[10.0, 0.0, 0.0], radius=2.0)
    assert info["context_index"].tolist() == [4, 6]


def test_design_argument_errors():
    rec = _line_receptor()
    ok = dict(center=[10.0, 0.0, 0.0])
    for bad in (dict(), dict(center=[0.0, 0.0, 0.0], hotspots=[1]), dict(center=[0.0, 0.0]), dict(center=[0.0, float("nan"), 0.0]),
                dict(hotspots=[]), dict(hotspots=[12]), dict(hotspots=[-1]), dict(hotspots=[1, 1]), dict(cavity={"center": 0}),
                dict(**ok, radius=0.0), dict(**ok, radius=float("inf")), dict(**ok, max_context=0), dict(**ok, max_context=509),
                dict(center=[500.0, 0.0, 0.0])):
        with pytest.raises(ValueError):
            design.make_design_batch(rec, 4, 1, **bad)
    for length, n in ((0, 1), (4, 0), (4.0, 1), (512, 1), (True, 1)):
        with pytest.raises(ValueError):
            design.make_design_batch(rec, length, n, **ok)
    with pytest.raises(TypeError):
        design.make_design_batch(rec, 4, 1, [10.0, 0.0, 0.0])                           # the site is keyword-only
