"""bench.py as it is run: the plain line (headline only, exactly --steps timed steps), --full (everything else the line carries),
--dump-outputs (the last timed step's outputs, identical from run to run and with or without --full)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("roofline", "roofline_other", "kernel_share_of_step", "final_state_check", "clocks_under_load", "whole_step_traffic",
             "secondary", "modes", "per_call", "cpu_baseline")
STATE = {"rotmats": (3, 3), "trans": (3,), "angles": (5,), "seqs": (), "seqs_simplex": (20,)}


def _bench(*args, timeout=900):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + [str(a) for a in args],
                       capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}


def test_plain_line_and_dumped_outputs(tmp_path):
    """Default workload (B = 64 x 128), plain run: the headline keys, none of the --full entries, value = residues x K / timed seconds;
    the dump is the sampler's final state, float32, a valid sample, and bit-identical from one process to the next."""
    K = 3
    a, b = tmp_path / "a", tmp_path / "b"
    out = _bench("--gpus", 1, "--steps", K, "--warmup", 1, "--dump-outputs", a)
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in out, k
    assert out["metric"] == "residues x denoise-steps / s" and out["unit"] == "res*step/s" and out["higher_is_better"] is True
    assert out["steps"] == K and out["warmup"] == 1 and out["ms_per_step"] > 0
    assert abs(out["value"] - 64 * 128 * K / (out["ms_per_step"] * K * 1e-3)) < 1e-6 * out["value"]
    assert not [k for k in FULL_ONLY if k in out], [k for k in FULL_ONLY if k in out]
    da = _load(a)
    assert set(da) == set(STATE)
    for k, tail in STATE.items():
        assert da[k].dtype == np.float32 and da[k].shape == (64, 128) + tail, (k, da[k].shape)
        assert np.isfinite(da[k]).all(), k
    R = da["rotmats"].astype(np.float64)
    assert np.abs(R @ R.transpose(0, 1, 3, 2) - np.eye(3)).max() < 1e-3
    assert ((da["seqs"] >= 0) & (da["seqs"] < 20) & (da["seqs"] == np.round(da["seqs"]))).all()
    _bench("--gpus", 1, "--steps", K, "--warmup", 1, "--dump-outputs", b)
    db = _load(b)
    for k in STATE:
        assert np.array_equal(da[k], db[k]), k


def test_full_line_keeps_its_entries_and_computes_the_same_outputs(tmp_path):
    """--full on cfg2: the per-kernel rooflines, the final-state check and the trajectory D2H are back, and the timed path's outputs
    are bit-identical to those of the plain run with the same arguments."""
    a, b = tmp_path / "plain", tmp_path / "full"
    common = ("--steps", 4, "--warmup", 2, "--workload", "cfg2")
    _bench(*common, "--dump-outputs", a)
    out = _bench(*common, "--full", "--no-cpu-baseline", "--dump-outputs", b)
    assert out["steps"] == 4
    for k in ("roofline", "roofline_other", "kernel_share_of_step", "final_state_check"):
        assert k in out, k
    assert out["roofline"]["avg_launch_us"] > 0 and out["final_state_check"]["det_err"] < 1e-3 and out["setup"]["d2h_steps"] == 6
    da, db = _load(a), _load(b)
    assert set(da) == set(db) == set(STATE)
    for k in STATE:
        assert da[k].shape[:2] == (16, 64) and np.array_equal(da[k], db[k]), k


def test_training_workload_dumps_losses_and_gradients(tmp_path):
    """cfg5: the dump holds the last timed step's six losses and one gradient per parameter, finite float32, within 64 MB."""
    d = tmp_path / "t"
    out = _bench("--workload", "cfg5", "--steps", 2, "--warmup", 1, "--dump-outputs", d)
    assert out["steps"] == 2 and out["ms_per_step"] > 0
    dd = _load(d)
    losses = {k for k in dd if not k.startswith("grad.")}
    assert losses == {"trans_loss", "rot_loss", "bb_atom_loss", "seqs_loss", "angle_loss", "torsion_loss"}, losses
    grads = [k for k in dd if k.startswith("grad.")]
    assert len(grads) > 100 and sum(dd[k].nbytes for k in dd) <= 64 << 20
    assert all(dd[k].dtype == np.float32 and np.isfinite(dd[k]).all() for k in dd)
    assert any(np.abs(dd[k]).max() > 0 for k in grads)
