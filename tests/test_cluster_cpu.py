"""CPU checks of the clustering layer: the ctypes struct against the header, the exported symbols and their argument checks, the
wrapper's argument checks, and the numpy oracle (cluster_oracle.py) itself -- its loop form against its vectorised form, the
constructed cases with hand-written answers, the linkages against scipy's fcluster(criterion="distance") as partitions, gromos'
defining properties, and the margin of the average linkage's merge heights to the cutoffs that the GPU tests rely on."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import cluster_cases as CC  # noqa: E402
import cluster_oracle as CO  # noqa: E402
from test_lddt_cpu import HEADER, header_fields  # noqa: E402
from pepflowww_amd import _capi, build, geometry, metrics  # noqa: E402

INT_KEYS = ("label", "cluster_size", "representative", "n_neighbours")


def test_struct_layout_agrees_with_the_header():
    assert [(n, t) for n, t in _capi.ClusterArgs._fields_] == header_fields("pf_cluster_args")
    assert _capi.ClusterArgs.cutoff.offset + 4 <= C.sizeof(_capi.ClusterArgs) and C.sizeof(_capi.ClusterArgs) % 8 == 0


def test_header_bound_and_insertion_points():
    text = open(HEADER).read()
    assert "#define PF_CLUSTER_MAX_N 1024" in text and geometry.CLUSTER_MAX_N == 1024
    assert geometry.CLUSTER_METHODS == ("gromos", "single", "complete", "average")
    assert "#define PF_ABI_VERSION 65" in text and _capi.ABI_VERSION == 65
    assert text.index("} pf_contacts_args;") < text.index("} pf_cluster_args;") < text.index("} pf_interface_energy_args;")
    assert build.SOURCES.index("clustering.hip") == build.SOURCES.index("contacts.hip") + 1
    syms = _capi.EXPORTED_SYMBOLS
    assert syms.index("pf_cluster_fwd") == syms.index("pf_contacts_fwd") + 1 == syms.index("pf_cluster_work_bytes") - 1


def test_library_exports_the_entry_points():
    lib = _capi.load()
    assert lib.pf_abi_version() == _capi.ABI_VERSION == 65
    assert lib.pf_cluster_fwd(None, None) == -1
    assert lib.pf_cluster_fwd(C.byref(_capi.ClusterArgs()), None) == -1
    assert lib.pf_cluster_work_bytes(1024, 0) == 0
    assert lib.pf_cluster_work_bytes(1024, 1) == lib.pf_cluster_work_bytes(1024, 2) == 4 * 1024 * 1024
    assert lib.pf_cluster_work_bytes(1024, 3) == 8 * 1024 * 1024 and lib.pf_cluster_work_bytes(7, 3) == 8 * 49
    assert lib.pf_cluster_work_bytes(1025, 1) == -1 and lib.pf_cluster_work_bytes(0, 1) == -1 and lib.pf_cluster_work_bytes(8, 4) == -1


def test_entry_point_refuses_bad_arguments_before_any_launch():
    """every pointer is a host buffer here: a call that got as far as a launch would not return an argument error"""
    lib = _capi.load()
    buf = (C.c_char * 64)()

    def args(**kw):
        a = _capi.ClusterArgs()
        for name, typ in _capi.ClusterArgs._fields_:
            if typ is C.c_void_p and name not in ("score", "best"):
                setattr(a, name, C.addressof(buf))
        a.B, a.G, a.n_max, a.method, a.cutoff = 4, 1, 4, 0, 1.0
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    for bad in (dict(B=0), dict(G=0), dict(n_max=0), dict(method=4), dict(method=-1), dict(cutoff=-1.0), dict(cutoff=float("nan")),
                dict(dist=None), dict(index=None), dict(offsets=None), dict(label=None), dict(n_clusters=None),
                dict(score=C.addressof(buf)), dict(method=2, work=None)):
        assert lib.pf_cluster_fwd(C.byref(args(**bad)), None) == -1, bad
    assert lib.pf_cluster_fwd(C.byref(args(n_max=1025)), None) == -2


def test_wrapper_argument_checks():
    d = torch.zeros(4, 4)
    for bad in (torch.zeros(4, 3), torch.zeros(4), torch.zeros(2, 2, 2), [[0.0]]):
        with pytest.raises(ValueError):
            geometry.cluster(bad, 1.0)
    with pytest.raises(ValueError):
        geometry.cluster(d, 1.0, method="ward")
    for cutoff in (float("nan"), -0.5):
        with pytest.raises(ValueError):
            geometry.cluster(d, cutoff)
    for score in (torch.zeros(3), torch.zeros(4, 1), [0.0] * 4):
        with pytest.raises(ValueError):
            geometry.cluster(d, 1.0, score=score)
    with pytest.raises(ValueError):
        geometry.cluster(d, 1.0, groups=[0, 0, 1])
    with pytest.raises(ValueError):                                 # a group of 1025, found on the host
        geometry.cluster(torch.zeros(1030, 1030), 1.0, groups=[0] * 1025 + [1] * 5)
    with pytest.raises(_capi.PepflowHipError):                      # CPU tensors: no fallback
        geometry.cluster(d, 1.0)
    with pytest.raises(_capi.PepflowHipError):
        geometry.cluster(d, 1.0, groups=[0, 0, 1, 1], method="average", score=torch.zeros(4))
    with pytest.raises(ValueError):
        metrics.cluster_samples({}, {}, metric="gdt")
    assert set(metrics.CLUSTER_CUTOFFS) == set(metrics.CLUSTER_METRICS)


def test_index_and_offsets_follow_the_groups():
    index, offsets, labels = CO.index_offsets([5, 2, 5, 9, 2, 5])
    assert index.tolist() == [1, 4, 0, 2, 5, 3] and offsets.tolist() == [0, 2, 5, 6] and labels.tolist() == [2, 5, 9]


@pytest.mark.parametrize("name,dist,cutoff,method,expected", CC.constructed(), ids=[c[0] for c in CC.constructed()])
@pytest.mark.parametrize("vectorised", [False, True])
def test_oracle_on_the_constructed_cases(name, dist, cutoff, method, expected, vectorised):
    n = dist.shape[0]
    got = CO.cluster(dist, np.arange(n), [0, n], cutoff, method, vectorised=vectorised)
    for k, v in expected.items():
        assert np.array_equal(np.asarray(got[k]).reshape(-1), np.asarray(v).reshape(-1)), (k, got[k], v)
    dirty = CO.cluster(CC.with_garbage_below(dist), np.arange(n), [0, n], cutoff, method, vectorised=vectorised)
    for k in INT_KEYS + ("n_clusters",):
        assert np.array_equal(dirty[k], got[k]), k


@pytest.mark.parametrize("method", CO.METHODS)
@pytest.mark.parametrize("n", CC.SIZES)
def test_vectorised_oracle_equals_the_loop_oracle(n, method):
    d = CO.group_matrix(CC.seeded_matrix(n), np.arange(n))
    score = CC.seeded_scores(n)
    for cutoff in CC.CUTOFFS:
        a = CO.cluster_group(d, cutoff, method, score, vectorised=False)
        b = CO.cluster_group(d, cutoff, method, score, vectorised=True)
        for k in INT_KEYS + ("best", "n_clusters"):
            assert np.array_equal(a[k], b[k]), (k, cutoff)
        assert a["heights"] == b["heights"] and a["refused"] == b["refused"]


def same_partition(a, b):
    pairs = set(zip(a.tolist(), b.tolist()))
    return len(pairs) == len(set(a.tolist())) == len(set(b.tolist()))


@pytest.mark.parametrize("method", ["single", "complete", "average"])
@pytest.mark.parametrize("n", CC.SCIPY_SIZES)
def test_linkages_agree_with_scipy_as_partitions(n, method):
    hierarchy = pytest.importorskip("scipy.cluster.hierarchy")
    squareform = pytest.importorskip("scipy.spatial.distance").squareform
    d = CC.seeded_matrix(n)
    Z = hierarchy.linkage(squareform(d.astype(np.float64), checks=False), method)
    for cutoff in CC.CUTOFFS:
        ours = CO.cluster_group(CO.group_matrix(d, np.arange(n)), cutoff, method)["label"]
        assert same_partition(ours, hierarchy.fcluster(Z, cutoff, "distance")), cutoff


def test_average_heights_keep_clear_of_the_cutoffs():
    """The GPU tests compare integer outputs without a tolerance.  The average linkage's heights are float64 sums and quotients: the
    kernel forms them in the written order without contraction, so they should agree to the last bit, and this margin makes sure
    that even a last-bit difference in a height could not move a cut in the inputs those tests use."""
    cases = [CC.mixed_batch()[0:2]] + [(CC.seeded_matrix(n), np.zeros(n, dtype=np.int64)) for n in CC.SIZES]
    for dist, groups in cases:
        index, offsets, _ = CO.index_offsets(groups)
        for cutoff in CC.CUTOFFS:
            o = CO.cluster(dist, index, offsets, cutoff, "average")
            hs = np.array(o["heights"] + [h for h in o["refused"] if np.isfinite(h)])
            assert hs.size == 0 or np.abs(hs - cutoff).min() > 1e-6 * max(1.0, cutoff), cutoff


@pytest.mark.parametrize("n", CC.SIZES)
def test_gromos_properties_of_the_oracle(n):
    d = CO.group_matrix(CC.seeded_matrix(n), np.arange(n))
    for cutoff in CC.CUTOFFS:
        o = CO.cluster_group(d, cutoff, "gromos")
        lab, size, rep = o["label"], o["cluster_size"], o["representative"]
        assert sorted(set(lab.tolist())) == list(range(o["n_clusters"]))                    # a partition, numbered without gaps
        sizes = np.bincount(lab)
        assert np.array_equal(sizes[lab], size) and np.all(np.diff(sizes) <= 0)             # sizes are non-increasing
        assert np.array_equal(lab[rep], lab) and np.array_equal(rep[rep], rep)              # the centre is a member, one per cluster
        centre = d[np.arange(n), rep]
        assert np.all((centre <= np.float32(cutoff)) | (rep == np.arange(n)))               # every member is within the cutoff of it
        rows = (d <= np.float32(cutoff)).sum(1) + (np.diag(d) > np.float32(cutoff))         # the row counts, self included
        assert np.array_equal(o["n_neighbours"], rows)
