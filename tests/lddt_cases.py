"""Seeded inputs and the comparison rules shared by test_gpu_lddt.py and test_gpu_dockq.py: test infrastructure.

The rule (derived, not tuned).  The kernels decide every atom pair in fp32 from the same coordinates as the float64 oracle, so a
decision whose float64 margin is below bound = 8 * 2^-23 * max|coord| (the ULP8 * mc of test_gpu_violations.py) may fall on the other
side, and no other: per row residue |scored - oracle| <= near_scored and |kept - oracle| <= near_kept + 4 near_scored (a pair that
changes sides at the cutoff takes up to four thresholds with it); contact counts likewise with their near counts.  The cap is a
condition on the case, stated on the oracle's numbers: its near pairs are at most 5e-4 of its scored pairs (of its contacts), so a
case that would need more is a bad case and fails."""
import numpy as np

import dssp_build as DB
import lddt_oracle as LO

ULP8 = 8.0 * 2.0 ** -23
NEAR_CAP = 5e-4


def make_pair_batch(rng, B, N, scale, mask_last_x=True):
    """-> x, y: dicts of pos [B,N,15,3] fp32, atom_mask [B,N,15] bool, aa [B,N] int64.  y: NeRF backbone segments of up to 30 residues
    placed at random within +-scale, side-chain atoms 1.5 - 4 A from CA; x[b] = y[b] plus Gaussian noise of 0.3 - 2 A (one sigma per
    structure), about a tenth of its residues of another type; masks with holes, drawn for each side on its own; the last structure
    of x all masked."""
    pos = np.zeros((B, N, 15, 3))
    for b in range(B):
        k = 0
        while k < N:
            n = int(min(N - k, rng.integers(1, 31)))
            seg = DB.random_chain(rng, n) @ DB.rotation(rng.standard_normal(3) * 2.0).T
            room = max(scale - 6.0 - np.abs(seg - seg.mean((0, 1))).max(), 0.0)
            if room == 0.0:
                seg = seg * (scale - 6.0) / np.abs(seg - seg.mean((0, 1))).max()
            pos[b, k:k + n, :4] = seg - seg.mean((0, 1)) + rng.uniform(-room, room, 3)
            k += n
        d = rng.standard_normal((N, 11, 3))
        pos[b, :, 4:] = pos[b, :, 1:2] + d / np.linalg.norm(d, axis=-1, keepdims=True) * rng.uniform(1.5, 4.0, (N, 11, 1))
    pos_y = np.clip(pos, -scale, scale).astype(np.float32)
    sigma = rng.uniform(0.3, 2.0, (B, 1, 1, 1))
    pos_x = np.clip(pos_y + sigma * rng.standard_normal(pos.shape), -scale - 8.0, scale + 8.0).astype(np.float32)
    aa_y = rng.integers(0, 21, size=(B, N)).astype(np.int64)
    aa_x = np.where(rng.random((B, N)) < 0.1, rng.integers(0, 21, size=(B, N)), aa_y).astype(np.int64)
    holes = lambda: (rng.random((B, N, 15)) > 0.1) & (rng.random((B, N, 1)) > 0.08)  # noqa: E731
    mask_x, mask_y = holes(), holes()
    if mask_last_x:
        mask_x[B - 1] = False
    return dict(pos=pos_x, atom_mask=mask_x, aa=aa_x), dict(pos=pos_y, atom_mask=mask_y, aa=aa_y)


def work_list(B):
    """every index of x and of y, a repeated pair, and indices out of range on either side"""
    ids = np.arange(B)
    pairs = np.stack([ids, (ids + 1) % B], 1).tolist() + [[0, 0], [0, 1 % B], [B, 0], [0, -1]]
    return np.array(pairs, np.int32)


def queries(rng, B, N):
    """query [B,N] of y: structure 0 without a residue, structure 1 with one residue in the last tile, the others a quarter"""
    q = rng.random((B, N)) < 0.25
    q[0] = False
    if B > 1:
        q[1] = np.arange(N) == N - 1
    return q


def bound_of(x, y):
    return ULP8 * float(max(np.abs(x["pos"][:, :, :14]).max(), np.abs(y["pos"][:, :, :14]).max()))


def in_range(pair, x, y):
    return 0 <= pair[0] < x["pos"].shape[0] and 0 <= pair[1] < y["pos"].shape[0]


def check_lddt(got, x, y, pairs, slot_mask, excl, query=None, group=None, cutoff=15.0):
    """got: the numpy outputs of geometry.lddt -> (scored pairs, near pairs) of the case"""
    bound = bound_of(x, y)
    tags = ("", "_cross") if group is not None else ("",)
    cache, n_scored, n_near = {}, 0, 0
    for p, (i, j) in enumerate(pairs.tolist()):
        if not in_range((i, j), x, y):
            for k in ("scored", "kept"):
                for t in tags:
                    assert not got[k + t][p].any(), (p, k + t)
            continue
        if (i, j) not in cache:
            cache[i, j] = LO.lddt(x["pos"][i], x["atom_mask"][i], x["aa"][i], y["pos"][j], y["atom_mask"][j], y["aa"][j], slot_mask, cutoff,
                                  excl, None if group is None else group[j], None if query is None else query[j], bound)
            n_scored += int(cache[i, j]["scored"].sum())
            n_near += int(cache[i, j]["near_scored"].sum() + cache[i, j]["near_kept"].sum())
        o = cache[i, j]
        for t in tags:
            ds = np.abs(got["scored" + t][p].astype(np.int64) - o["scored" + t])
            dk = np.abs(got["kept" + t][p].astype(np.int64) - o["kept" + t])
            assert (ds <= o["near_scored" + t]).all(), (p, i, j, "scored" + t, int(ds.max()))
            assert (dk <= o["near_kept" + t] + 4 * o["near_scored" + t]).all(), (p, i, j, "kept" + t, int(dk.max()))
            if "scored_atom" + t in got:
                assert np.array_equal(got["scored_atom" + t][p].sum(-1), got["scored" + t][p]), (p, t)
                assert np.array_equal(got["kept_atom" + t][p].sum(-1), got["kept" + t][p]), (p, t)
                if not o["near_scored" + t].any() and not o["near_kept" + t].any():
                    assert np.array_equal(got["scored_atom" + t][p], o["scored_atom" + t]), (p, t)
                    assert np.array_equal(got["kept_atom" + t][p], o["kept_atom" + t]), (p, t)
        if query is not None:
            assert not got["scored"][p][~query[j]].any() and not got["kept"][p][~query[j]].any(), p
        with np.errstate(invalid="ignore", divide="ignore"):
            assert np.array_equal(got["lddt_residue"][p], got["kept"][p] / (4.0 * got["scored"][p]), equal_nan=True)
    assert n_near <= NEAR_CAP * n_scored, ("a bad case: too many decisions near a threshold", n_near, n_scored)
    return n_scored, n_near


def check_contacts(got, x, y, pairs, group, slot_mask=0x3FFF, contact_cutoff=5.0, interface_cutoff=10.0):
    """got: the numpy outputs of geometry.interface_contacts -> (contacts, near residue pairs) of the case"""
    bound = ULP8 * float(max(np.abs(x["pos"]).max(), np.abs(y["pos"]).max()))
    cache, n_contacts, n_near = {}, 0, 0
    for p, (i, j) in enumerate(pairs.tolist()):
        if not in_range((i, j), x, y):
            for k in ("contacts_x", "contacts_y", "contacts_shared", "interface_x", "interface_y"):
                assert not got[k][p].any(), (p, k)
            assert np.isinf(got["min_dist_x"][p]).all() and np.isinf(got["min_dist_y"][p]).all()
            continue
        if (i, j) not in cache:
            cache[i, j] = LO.contacts(x["pos"][i], x["atom_mask"][i], y["pos"][j], y["atom_mask"][j], group[j], slot_mask, contact_cutoff,
                                      interface_cutoff, bound)
            n_contacts += int(cache[i, j]["contacts_x"].sum() + cache[i, j]["contacts_y"].sum())
            n_near += int(cache[i, j]["near_contact_x"].sum() + cache[i, j]["near_contact_y"].sum())
        o = cache[i, j]
        for t in ("x", "y"):
            d = np.abs(got["contacts_" + t][p].astype(np.int64) - o["contacts_" + t])
            assert (d <= o["near_contact_" + t]).all(), (p, i, j, "contacts_" + t, int(d.max()))
            diff = got["interface_" + t][p] != o["interface_" + t]
            assert not (diff & (o["near_interface_" + t] == 0)).any(), (p, i, j, "interface_" + t)
            mine, ref = got["min_dist_" + t][p].astype(np.float64), o["min_dist_" + t]
            assert np.array_equal(np.isinf(mine), np.isinf(ref)), (p, i, j, "min_dist_" + t)
            fin = np.isfinite(ref)
            # float_bound of test_gpu_violations.py with one term: 8 ulp of the largest coordinate per term (+ 1), 1e-6 relative
            assert (np.abs(mine[fin] - ref[fin]) <= bound * 2 + 1e-6 * ref[fin]).all(), (p, i, j, "min_dist_" + t)
        d = np.abs(got["contacts_shared"][p].astype(np.int64) - o["contacts_shared"])
        assert (d <= o["near_contact_x"] + o["near_contact_y"]).all(), (p, i, j, "contacts_shared")
    assert n_near <= NEAR_CAP * n_contacts, ("a bad case: too many residue pairs near the cutoff", n_near, n_contacts)
    return n_contacts, n_near
