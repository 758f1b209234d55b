"""Shapes, seeds and file layout of the golden fixtures F17 - F19: arrays recorded from the REFERENCE at the lengths where the
denoise engine and the training step run their production plans (64 <= L <= 256 and the edges around it), not only at L <= 32 as
F2 - F6.  Shared by the generators (tests/golden/make_golden_f17.py, _f18, _f19), tests/test_oracle_golden.py and
tests/test_gpu_reference_shapes.py.  Pure bookkeeping: nothing here runs a model.

A fixture is a set of part files `<stem>_<part>.npz` (every committed file stays below 1 MiB); load_parts() merges them.
"""
import glob
import io
import os
import zipfile

import numpy as np
import torch

from pepflowww_amd import synth

N_GEN = 10
MAX_FILE_BYTES = 1 << 20

# F17, one denoise step per plan class: (B, L, lengths)
F17_SHAPES = [(2, 64, [64, 51]), (2, 128, [128, 97]), (1, 68, [61]), (1, 70, [70]), (1, 144, [137]), (1, 272, [259])]
# F18, 3-step sample() with recorded RNG
F18_SHAPES = [(2, 64, [64, 51]), (2, 128, [128, 97]), (1, 144, [137])]
F18_STEPS = 3
F18_FIRST_NOISE_SEED = 99
F18_MIN_MARGIN = 2e-3          # smallest relative top-2 gap of a categorical draw on a generated row: 20 x the 1e-4 parity bar
# F19, one training step
F19_SHAPES = [(2, 64, [64, 51]), (2, 128, [128, 97])]
F19_LOOSE_NOISE = 3.2e-3       # tests/train_oracle.py: LOOSE_NOISE
F19_MAX_LOOSE = 20             # tests/test_gpu_train_shapes.py: MAX_LOOSE
F19_DISTCOEF = "edge_embedder.aapair_to_distcoef.weight"
ORACLE_CEILING = 2e-5          # reference vs restatement after one step, any tensor (max-normalised; angles in rad)

NOISE_KEYS = ("rot0", "trans0", "ang0", "simplex0", "expo")
TRAIN_NOISE_KEYS = ("t", "trans0", "rot0", "ang0", "simplex0", "expo")


def tag(B, L):
    return f"b{B}_l{L}"


def f17_batch(B, L, lengths):
    return synth.make_pocket_batch(B, L, N_GEN, seed=1700 + L, lengths=lengths)


def f17_case_seed(L):
    return 170 + L


def f18_batch(B, L, lengths):
    return synth.make_pocket_batch(B, L, N_GEN, seed=777 + L, lengths=lengths)


def f19_batch(B, L, lengths, cand=0):
    return synth.make_pocket_batch(B, L, N_GEN, seed=1900 + L + 1000 * cand, lengths=lengths)


def f19_noise_seed(L, cand=0):
    return 190 + L + 1000 * cand


def query_rows(L, lengths):
    """[B, 9] query rows i whose pair rows (all j, all channels) a fixture keeps: both sides of the 16-row tile edge, the middle,
    the last two valid rows and the last (possibly padded) row of each sample."""
    return torch.tensor([[0, 1, 15, 16, 17, L // 2, n - 2, n - 1, L - 1] for n in lengths], dtype=torch.int64)


def take_rows(pair, rows):
    """pair [B, L, L, C], rows [B, R] -> [B, R, L, C]."""
    return torch.stack([pair[b, rows[b]] for b in range(pair.shape[0])], 0)


def batch_of(f, prefix="batch_"):
    return {k[len(prefix):]: v for k, v in f.items() if k.startswith(prefix)}


def save_parts(golden_dir, stem, parts):
    """parts: {part name: {array name: tensor / array}}.  Written with fixed zip timestamps, so that a re-run reproduces the
    files byte for byte.  Returns [(file name, bytes)]."""
    sizes = []
    for part, arrs in parts.items():
        name = f"{stem}_{part}.npz"
        path = os.path.join(golden_dir, name)
        with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
            for k, v in arrs.items():
                a = v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)
                buf = io.BytesIO()
                np.lib.format.write_array(buf, np.ascontiguousarray(a), allow_pickle=False)
                info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
                info.compress_type = zipfile.ZIP_DEFLATED
                zf.writestr(info, buf.getvalue())
        n = os.path.getsize(path)
        assert n <= MAX_FILE_BYTES, (name, n)
        sizes.append((name, n))
    return sizes


def load_parts(golden_dir, stem):
    out = {}
    paths = sorted(glob.glob(os.path.join(golden_dir, stem + "_*.npz")))
    assert paths, stem
    for p in paths:
        d = np.load(p)
        for k in d.files:
            assert k not in out, (p, k)
            out[k] = torch.from_numpy(d[k])
    return out


def maxnorm(a, b):
    """max|a - b| / max|b|: the project's parity metric."""
    a, b = a.double(), b.double()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def circle(a, b):
    d = (a.double() - b.double()).abs()
    return torch.minimum(d, 2 * torch.pi - d).max().item()
