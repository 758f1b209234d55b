"""CPU checks of the structural-violation metric: the numpy float64 oracle (violation_oracle.py) against the fixture recorded from
the reference's OpenFold functions (golden F14), its `query` / `group` against a dense form with the masks applied, the package's
radius / slot / proline tables against the recorded ones, the wrapper's residue-index rule and argument checks, the C ABI's bounds."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import violation_oracle as VO  # noqa: E402
from pepflowww_amd import _capi, geometry, metrics  # noqa: E402
from pepflowww_amd.preprocess import _tables, residue_type  # noqa: E402

ULP8 = 8.0 * 2.0 ** -23


@pytest.fixture(scope="module")
def gold(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "f14_violations.npz")))


def float_bound(max_coord, terms, value, factor=1.0):
    """the derived bound: 8 ulp of the largest coordinate per nonzero term (+ 1) absolute, plus 1e-6 relative"""
    return factor * (ULP8 * max_coord * (np.asarray(terms) + 1) + 1e-6 * np.abs(value))


def oracle_row(g, s, **kw):
    return VO.violations(g["pos"][s], g["atom_mask"][s], g["aa"][s], g["residue_index"][s], g["radius"], int(g["pro"]), **kw)


PAIRS = [("clash_atom_loss", "ref_clash_per_atom_loss_sum", "clash_atom_terms"), ("clash_mean_loss", "ref_clash_mean_loss", "clash_mean_terms"),
         ("bond_c_n_loss_mean", "ref_bond_c_n_loss_mean", "bond_c_n_terms"), ("angle_ca_c_n_loss_mean", "ref_bond_ca_c_n_loss_mean", "angle_ca_c_n_terms"),
         ("angle_c_n_ca_loss_mean", "ref_bond_c_n_ca_loss_mean", "angle_c_n_ca_terms"),
         ("connection_loss", "ref_bond_per_residue_loss_sum", "connection_terms")]


def test_fixture_holds_what_it_promises(gold):
    for k in ("ref_clash_per_atom_clash_mask", "ref_bond_per_residue_violation_mask", "ca_ca_break"):
        assert 0.05 <= np.mean(gold[k] > 0) <= 0.95, k
    assert not gold["ref_bond_per_residue_violation_mask"][0].any()
    assert gold["min_margin"] >= 1e-3
    assert os.path.getsize(os.path.join(os.path.dirname(__file__), "golden", "f14_violations.npz")) < 400 * 1024


def test_oracle_matches_the_reference_fixture(gold):
    S = gold["pos"].shape[0]
    for s in range(S):
        o = oracle_row(gold, s)
        mc = np.abs(gold["pos"][s]).max()
        assert np.array_equal(o["clash_atom"], gold["ref_clash_per_atom_clash_mask"][s] > 0), s
        assert np.array_equal(o["connection_violation"], gold["ref_bond_per_residue_violation_mask"][s] > 0), s
        assert np.array_equal(o["ca_ca_break"], gold["ca_ca_break"][s]), s
        assert min(o["clash_atom_margin"].min(), o["connection_margin"].min(), o["ca_ca_margin"].min()) >= gold["min_margin"] - 1e-12
        for mine, ref, terms in PAIRS:
            err = np.abs(o[mine] - gold[ref][s].astype(np.float64))
            assert (err <= float_bound(mc, o[terms], o[mine], 2.0)).all(), (s, mine, err.max())
        n_conn = np.isfinite(o["ca_ca_margin"]).sum()
        assert abs(o["ca_ca_extreme"] - gold["ref_extreme_ca_ca"][s]) <= float_bound(mc, o["ca_ca_break"].sum(), o["ca_ca_extreme"], 2.0), s
        assert abs(o["ca_ca_extreme"] - o["ca_ca_break"].sum() / (1e-4 + n_conn)) <= 1e-15


def test_batched_reference_call_equals_the_rows(gold):
    """the reference's batched call (case e) gives the per-row values for everything but the mean clash loss, which it pools"""
    rows = gold["batch_rows"]
    for k in ("bond_c_n_loss_mean", "bond_per_residue_loss_sum", "bond_per_residue_violation_mask", "clash_per_atom_loss_sum",
              "clash_per_atom_clash_mask", "extreme_ca_ca"):
        assert np.allclose(gold["batched_" + k], gold["ref_" + k][rows], rtol=1e-5, atol=1e-5), k


def dense(pos, exists, radius, index, tol=1.5):
    """[N,N,14,14] pair arrays written as the reference writes them (both orders kept): counted, e, hit"""
    N = pos.shape[0]
    d = np.sqrt(1e-10 + ((pos[:, None, :, None, :] - pos[None, :, None, :, :]) ** 2).sum(-1))
    m = exists[:, None, :, None] & exists[None, :, None, :] & (index[:, None, None, None] != index[None, :, None, None])
    s = np.arange(14)
    cn = (index[:, None] + 1 == index[None, :])[:, :, None, None] & (s == 2)[None, None, :, None] & (s == 0)[None, None, None, :]
    m &= ~cn & ~cn.transpose(1, 0, 3, 2)
    m &= ~((s == 5)[None, None, :, None] & (s == 5)[None, None, None, :])
    lim = radius[:, None, :, None] + radius[None, :, None, :] - tol
    return m, np.where(m, np.maximum(lim - d, 0.0), 0.0), m & (d < lim)


@pytest.mark.parametrize("s", [3, 4, 5])
def test_query_and_group_against_the_dense_form(gold, s):
    rng = np.random.default_rng(70 + s)
    N = gold["pos"].shape[1]
    pos, exists = gold["pos"][s].astype(np.float64), gold["atom_mask"][s]
    index = gold["residue_index"][s].astype(np.int64)
    radius = np.where(exists, gold["radius"][gold["aa"][s]].astype(np.float64), 0.0)
    m, e, hit = dense(pos, exists, radius, index)
    peptide = np.arange(N) >= 40
    for query, group in ((peptide, peptide), (rng.random(N) < 0.3, rng.random(N) < 0.5), (None, peptide), (peptide, None),
                         (np.zeros(N, bool), peptide)):
        o = oracle_row(gold, s, query=query, group=group)
        q = np.ones((N, N), bool) if query is None else query[:, None] | query[None, :]
        mq, eq, hq = m & q[:, :, None, None], e * q[:, :, None, None], hit & q[:, :, None, None]
        assert np.array_equal(o["clash_atom_pairs"], mq.sum((1, 3)))
        assert np.allclose(o["clash_atom_loss"], eq.sum((1, 3)), rtol=0, atol=1e-12)
        assert np.array_equal(o["clash_atom"], hq.any((1, 3)))
        assert abs(o["clash_mean_loss"] - 0.5 * eq.sum() / (1e-6 + 0.5 * mq.sum())) <= 1e-15
        if group is None:
            assert "clash_atom_cross" not in o
        else:
            c = (group[:, None] != group[None, :])[:, :, None, None]
            assert np.allclose(o["clash_atom_loss_cross"], (eq * c).sum((1, 3)), rtol=0, atol=1e-12)
            assert np.array_equal(o["clash_atom_cross"], (hq & c).any((1, 3)))
        if query is not None and not query.any():
            assert o["clash_atom_pairs"].sum() == 0 and o["clash_mean_loss"] == 0.0


def test_package_tables_equal_the_recorded_ones(gold):
    tab = geometry.vdw_radius_table().numpy()
    assert tab.shape == (21, 14) and tab.dtype == np.float32
    assert np.array_equal(tab[:20], gold["radius"][:20])
    assert np.array_equal(tab[:20], gold["radius_openfold"][gold["pkg_to_openfold"][:20]])
    assert np.array_equal(tab[20], np.array([1.55, 1.7, 1.7, 1.52] + [0.0] * 10, np.float32))
    assert residue_type("PRO") == int(gold["pro"]) and gold["pkg_to_openfold"][int(gold["pro"])] == int(gold["pro_openfold"])
    names = _tables()["atom_names"]
    for t in range(20):
        assert names[t][:4] == ["N", "CA", "C", "O"]
        assert [bool(n) for n in names[t][:14]] == list(gold["radius"][t] > 0)
    assert names[residue_type("CYS")][5] == "SG"
    # the constants of the connection pass, as the kernel and the oracle spell them
    assert tuple(gold["bond_length_c_n"]) == VO.CN_LEN and tuple(gold["bond_length_stddev_c_n"]) == VO.CN_SD
    assert tuple(gold["cos_angles_ca_c_n"])[0] == VO.COS_CA_C_N and tuple(gold["cos_angles_c_n_ca"]) == (VO.COS_C_N_CA, VO.COS_C_N_CA_SD)
    assert float(gold["ca_ca"]) == VO.CA_CA and geometry.VDW_RADIUS == VO.VDW


def test_residue_index_rule():
    chain = torch.tensor([[0, 0, 0, 0, 1, 1, 1, 1], [0, 0, 0, 0, 0, 0, 0, 0]])
    res_nb = torch.tensor([[5, 6, 8, 9, 1, 2, 3, 4], [1, 2, 3, 4, 5, 5, 6, 7]])
    mask = torch.ones(2, 8, dtype=torch.bool)
    mask[1, 2] = False
    idx = metrics.residue_index(chain, res_nb, mask)
    assert idx.dtype == torch.int32
    # row 0: a numbering gap between 6 and 8 (+2), a chain change (+2); row 1: a masked residue (+2 on both sides), a repeated number (+2)
    assert idx.tolist() == [[0, 1, 3, 4, 6, 7, 8, 9], [0, 1, 3, 5, 6, 8, 9, 10]]
    assert (idx[:, 1:] > idx[:, :-1]).all()


def test_wrapper_argument_checks():
    pos = torch.zeros(2, 5, 14, 3)
    ok = dict(atom_mask=torch.ones(2, 5, 14, dtype=torch.bool), aa=torch.zeros(2, 5, dtype=torch.int64),
              residue_index=torch.arange(5).repeat(2, 1))
    with pytest.raises(ValueError):
        geometry.structural_violations(torch.zeros(2, 5, 4, 3), torch.ones(2, 5, 4, dtype=torch.bool), ok["aa"], ok["residue_index"])
    with pytest.raises(ValueError):
        geometry.structural_violations(pos, ok["atom_mask"][:, :, :4], ok["aa"], ok["residue_index"])
    with pytest.raises(ValueError):
        geometry.structural_violations(pos, **ok, query=torch.ones(2, 4, dtype=torch.bool))
    with pytest.raises(_capi.PepflowHipError):              # CPU tensors: no fall-back
        geometry.structural_violations(pos, **ok)
    with pytest.raises(ValueError):
        metrics.structural_violations({}, {}, backbone="atoms")
    with pytest.raises(ValueError):
        metrics.structural_violations({}, {}, scope="some")


def test_c_abi_bounds():
    assert _capi.ABI_VERSION == 65
    lib = _capi.load()
    assert lib.pf_abi_version() == 65
    a = _capi.ViolationsArgs()
    assert lib.pf_violations_fwd(C.byref(a), None) == -1
    assert lib.pf_violations_fwd(None, None) == -1
