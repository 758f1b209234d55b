"""Device-resident Euler sampler (FlowModel.sample loop, flow_model.py:279-374).

The reference syncs with the host nine times per step (`.cpu()` into clean_traj, 313-314) and
rebuilds `t` on the host every step (288).  Here the whole loop lives on the GPU:
  * state (R_t, x_t, angles_t, seq_t, simplex_t), the time grid and a step counter are device
    buffers; one step = DenoiseEngine plan + pf_sampler_step;
  * that step is captured ONCE into a hipGraph and replayed num_steps times (launch-bound inner
    loop -> one graph launch per step);
  * every step's clean prediction is written into [num_steps, ...] trajectory buffers; a single
    D2H copy at the end produces the reference's list of dicts of CPU tensors.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _capi


def quat_to_rot_host(q):
    """Unit quaternions [..., 4] -> rotation matrices [..., 3, 3] on the host, in NUMPY: torch's CPU ops fork an OpenMP team for any
    tensor beyond 32 k elements, and in a process whose (often > 100) pool threads were used elsewhere that fork was measured at 20 - 200 ms
    for a 150 KB tensor (profiles/r05/README.md, per-call stalls) -- numpy's elementwise loops stay on the calling thread."""
    import numpy as np
    q = q.numpy() if torch.is_tensor(q) else q
    q = q / np.sqrt((q * q).sum(-1, keepdims=True))
    a, b, c, d = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    rot = np.stack([a*a+b*b-c*c-d*d, 2*(b*c-a*d), 2*(b*d+a*c),
                    2*(b*c+a*d), a*a-b*b+c*c-d*d, 2*(c*d-a*b),
                    2*(b*d-a*c), 2*(c*d+a*b), a*a-b*b-c*c+d*d], -1).astype(np.float32)
    return torch.from_numpy(np.ascontiguousarray(rot.reshape(q.shape[:-1] + (3, 3))))


def default_noise(B, L, generator=None):
    """Initial noise drawn on the host like the reference's uniform_so3 (pepflow/modules/so3/dist.py:40-45,
    Haar via normalised Gaussian quaternions) + randn / rand (flow_model.py:255,264,269)."""
    g = generator
    q = torch.randn(B, L, 4, generator=g)                 # (draw order as before: rotations, translations, angles, simplex)
    trans0 = torch.randn(B, L, 3, generator=g)
    ang = torch.rand(B, L, 5, generator=g)
    return {"rot0": quat_to_rot_host(q), "trans0": trans0, "ang0": torch.from_numpy(ang.numpy() * np.float32(2 * math.pi)),
            "simplex0": torch.randn(B, L, 20, generator=g)}


# ---- conditioned sampling: host-side validation and packing (no GPU needed) ------------------------------------------------------
# The reference's sample() (flow_model.py:229-374) has none of this: it starts from pure noise on linspace(1e-2, 1, num_steps), its three
# switches cover the whole peptide, and any of the 20 residue types may be drawn.  A partial start places the initial state on the
# training corruption's interpolants (flow_model.py:125-158) between the noise and a given state: an OFF-LABEL use of the trained flow.
ALL_AA = (1 << 20) - 1                       # every class allowed (pf_sampler_cond_args.aa_allowed)
FLAG_BB, FLAG_ANG, FLAG_SEQ = 1, 2, 4        # bits of pf_sampler_cond_args.res_flags
_START_KEYS = {"rotmats": (3, 3), "trans": (3,), "angles": (5,), "seqs": ()}      # the entries of a trajectory dict a start may give
COND_ROW_KEYS = ("res_flags", "aa_allowed") + tuple(_START_KEYS)                  # the per-residue tensors of a packed `cond`
_COND_PAD = {"res_flags": 0, "aa_allowed": ALL_AA, "rotmats": 0, "trans": 0, "angles": 0, "seqs": 21}


def make_grid(num_steps, t_start=None, ts=None):
    """The time grid of a call as an fp32 CPU tensor [num_steps]: linspace(1e-2, 1, N) (flow_model.py:280), linspace(t_start, 1, N) for
    0 < t_start < 1, or the caller's own strictly increasing `ts` in (0, 1].  ValueError otherwise."""
    num_steps = int(num_steps)
    if num_steps < 1:
        raise ValueError(f"num_steps = {num_steps}: at least one step")
    if ts is not None:
        if t_start is not None:
            raise ValueError("t_start and ts exclude each other: ts IS the grid")
        g = torch.as_tensor(ts).detach().to("cpu", torch.float32)
        if g.dim() != 1 or g.numel() != num_steps:
            raise ValueError(f"ts: expected a 1-D grid of num_steps = {num_steps} values, got shape {tuple(g.shape)}")
        if not (bool(g[0] > 0) and bool(g[-1] <= 1) and bool((g[1:] > g[:-1]).all())):
            raise ValueError("ts: expected strictly increasing values in (0, 1]")
        return g.clone().contiguous()
    if t_start is None:
        return torch.linspace(1e-2, 1.0, num_steps)
    t = float(t_start)
    if not 0.0 < t < 1.0:
        raise ValueError(f"t_start = {t_start}: expected 0 < t_start < 1")
    return torch.linspace(t, 1.0, num_steps)


def pack_res_flags(sample_bb, sample_ang, sample_seq, B, L):
    """-> (scalar flags, byte plane).  All three plain bools: (the bools, None).  Any bool [B, L] tensor among them: the scalars are
    broadcast and the call runs on the uint8 [B, L] plane (bit 0 backbone, 1 angles, 2 sequence); the scalar flags are then unused
    by the kernels and returned as all-True (one cached sampler serves every plane)."""
    vals = (sample_bb, sample_ang, sample_seq)
    if not any(torch.is_tensor(v) for v in vals):
        return tuple(bool(v) for v in vals), None
    plane = np.zeros((B, L), dtype=np.uint8)
    for bit, (name, v) in enumerate(zip(("sample_bb", "sample_ang", "sample_seq"), vals)):
        if torch.is_tensor(v):
            if v.dtype != torch.bool or tuple(v.shape) != (B, L):
                raise ValueError(f"{name}: expected a bool or a bool tensor [{B}, {L}], got {v.dtype} {tuple(v.shape)}")
            m = v.detach().cpu().numpy()
        else:
            m = np.full((B, L), bool(v))
        plane |= m.astype(np.uint8) << np.uint8(bit)
    return (True, True, True), torch.from_numpy(plane)


def pack_aa_allowed(aa_allowed, B, L):
    """bool [20] / [L, 20] / [B, L, 20] -> int32 [B, L] with bit k = class k may be drawn; None -> None.  A row that allows no class
    raises ValueError."""
    if aa_allowed is None:
        return None
    m = torch.as_tensor(aa_allowed)
    if m.dtype != torch.bool or m.dim() not in (1, 2, 3) or tuple(m.shape) != (B, L, 20)[3 - m.dim():]:
        raise ValueError(f"aa_allowed: expected bool [20], [{L}, 20] or [{B}, {L}, 20], got {m.dtype} {tuple(m.shape)}")
    a = np.broadcast_to(m.detach().cpu().numpy(), (B, L, 20))
    bits = (a.astype(np.int64) << np.arange(20, dtype=np.int64)).sum(-1).astype(np.int32)
    if (bits == 0).any():
        b, l = np.argwhere(bits == 0)[0]
        raise ValueError(f"aa_allowed: no class allowed at sample {b}, residue {l}")
    return torch.from_numpy(np.ascontiguousarray(bits))


def check_start(start, B, L):
    """None -> None (pure noise); "native" -> {} (every entry from the batch's own peptide); a dict with any of rotmats [B,L,3,3],
    trans [B,L,3], angles [B,L,5], seqs [B,L] (the entries of a trajectory dict; others are ignored, a missing one takes the
    native's value) -> those entries as fp32 / int64 tensors on the device they came from.  seqs outside 0..21 raise (for a device
    tensor that is one host read of its extremes)."""
    if start is None:
        return None
    if isinstance(start, str):
        if start != "native":
            raise ValueError(f"start = {start!r}: expected None, 'native' or a dict")
        return {}
    if not isinstance(start, dict):
        raise ValueError(f"start: expected None, 'native' or a dict, got {type(start).__name__}")
    out = {}
    for k, tail in _START_KEYS.items():
        v = start.get(k)
        if v is None:
            continue
        if not torch.is_tensor(v) or tuple(v.shape) != (B, L) + tail:
            raise ValueError(f"start[{k!r}]: expected a tensor {(B, L) + tail}, got {tuple(v.shape) if torch.is_tensor(v) else type(v).__name__}")
        if k == "seqs":
            if v.dtype not in (torch.int64, torch.int32):
                raise ValueError(f"start['seqs']: expected an integer tensor, got {v.dtype}")
            # residue types 0..19; 20 (UNK) and 21 (PAD) as a batch's `aa` may hold them on context rows: like seq_to_simplex
            # (flow_model.py:108-109) they give the simplex of no class.  Anything else is a mistake, not a residue type.
            if v.numel() and not (0 <= int(v.min()) and int(v.max()) <= 21):
                raise ValueError(f"start['seqs']: residue types must lie in 0..21, got {int(v.min())}..{int(v.max())}")
            out[k] = v.detach().to(torch.int64)
        else:
            if not v.dtype.is_floating_point:
                raise ValueError(f"start[{k!r}]: expected a floating-point tensor, got {v.dtype}")
            out[k] = v.detach().to(torch.float32)
    return out


def make_cond(B, L, num_steps, sample_bb=True, sample_ang=True, sample_seq=True, t_start=None, ts=None, start=None, aa_allowed=None):
    """Everything sample()'s conditioning arguments say, validated: (grid, scalar flags, cond).  cond is None for a call that uses none
    of them beyond the grid, else a dict: "partial" (bool) and any of the per-residue tensors COND_ROW_KEYS at the caller's [B, L]."""
    grid = make_grid(num_steps, t_start, ts)
    flags, plane = pack_res_flags(sample_bb, sample_ang, sample_seq, B, L)
    allowed = pack_aa_allowed(aa_allowed, B, L)
    st = check_start(start, B, L)
    if st is not None and t_start is None and ts is None:
        raise ValueError("start needs a grid: pass t_start or ts (the state is placed at the grid's first time)")
    if plane is None and allowed is None and st is None:
        return grid, flags, None
    cond = {"partial": st is not None}
    if plane is not None:
        cond["res_flags"] = plane
    if allowed is not None:
        cond["aa_allowed"] = allowed
    cond.update(st or {})
    return grid, flags, cond


def fit_cond(cond, L0, Lk, idx=None):
    """The packed conditioning of the samples `idx` (None: all) with the residue axis cut or padded from L0 to Lk by INERT rows: no
    flag set, every class allowed, identity frame, zeros, residue type 21 (none of it is read: padded rows are not generated)."""
    if cond is None:
        return None
    from .buckets import _fit, _rows
    out = {"partial": cond["partial"]}
    for k in COND_ROW_KEYS:
        v = cond.get(k)
        if v is None:
            continue
        w = _fit(v if idx is None else _rows(v, idx), L0, Lk, 1, _COND_PAD[k])
        if k == "rotmats" and Lk > L0:
            for d in range(3):
                w[:, L0:, d, d] = 1
        out[k] = w
    return out


def shard_cond_kwargs(kw, lo, hi, total):
    """sample()'s conditioning keywords with every per-sample tensor ([total, ...]) cut to the shard [lo, hi)."""
    out = dict(kw)
    for k in ("sample_bb", "sample_ang", "sample_seq"):
        if torch.is_tensor(out.get(k)) and out[k].dim() == 2 and out[k].shape[0] == total:
            out[k] = out[k][lo:hi]
    a = out.get("aa_allowed")
    if a is not None and torch.as_tensor(a).dim() == 3 and torch.as_tensor(a).shape[0] == total:
        out["aa_allowed"] = torch.as_tensor(a)[lo:hi]
    if isinstance(out.get("start"), dict):
        out["start"] = {k: (v[lo:hi] if k in _START_KEYS and torch.is_tensor(v) and v.dim() >= 2 and v.shape[0] == total else v)
                        for k, v in out["start"].items()}
    return out


class DeviceSampler:
    """Owned by its engine (DenoiseEngine.sampler caches one per (num_steps, flags, cond)): trajectory buffers and the captured graphs are
    reused by the next sample() call; set_seed() / set_grid() / set_context() / set_cond() / init_state() are what a call changes."""

    def __init__(self, engine, num_steps, flags=(True, True, True), first_sample=0, seed=0, cond=False):
        self.eng = engine
        self.lib = engine.lib
        self.N = num_steps
        B, L, dev = engine.B, engine.L, engine.device
        rows = B * L
        e = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)
        self.rot1, self.trans1, self.ang1 = e(rows, 9), e(rows, 3), e(rows, 5)
        self.seq1 = e(rows, dt=torch.int64)
        self.gen = e(rows)
        self.simplex_t, self.trans0, self.simplex0 = e(rows, 20), e(rows, 3), e(rows, 20)
        self.traj_rot, self.traj_trans = e(num_steps, rows, 9), e(num_steps, rows, 3)
        self.traj_ang, self.traj_simplex = e(num_steps, rows, 5), e(num_steps, rows, 20)
        self.traj_seq = e(num_steps, rows, dt=torch.int64)
        self.ts = torch.linspace(1e-2, 1.0, num_steps).to(dev)          # flow_model.py:280 (built on CPU, then H2D)
        self.step = e(2, dt=torch.int32)                      # [0] step counter, [1] workgroup ticket
        self.expo = None
        a = _capi.SamplerArgs()
        a.rot1, a.trans1, a.ang1, a.seq1 = self.rot1.data_ptr(), self.trans1.data_ptr(), self.ang1.data_ptr(), self.seq1.data_ptr()
        a.gen_mask, a.res_mask = self.gen.data_ptr(), engine.mask.data_ptr()
        a.rot_t, a.trans_t, a.ang_t, a.seq_t = engine.rot_t.data_ptr(), engine.trans_t.data_ptr(), engine.ang_t.data_ptr(), engine.seq_t.data_ptr()
        a.simplex_t, a.trans0, a.simplex0 = self.simplex_t.data_ptr(), self.trans0.data_ptr(), self.simplex0.data_ptr()
        a.pred_rot, a.pred_trans = engine.rot.data_ptr(), engine.trans.data_ptr()
        a.pred_ang_raw, a.pred_logits = engine.ang_raw.data_ptr(), engine.logits.data_ptr()
        a.traj_rot, a.traj_trans, a.traj_ang = self.traj_rot.data_ptr(), self.traj_trans.data_ptr(), self.traj_ang.data_ptr()
        a.traj_seq, a.traj_simplex = self.traj_seq.data_ptr(), self.traj_simplex.data_ptr()
        a.ts, a.num_steps, a.step, a.t_out = self.ts.data_ptr(), num_steps, self.step.data_ptr(), engine.t.data_ptr()
        a.expo, a.seed, a.first_sample = None, seed & (2 ** 64 - 1), first_sample
        a.B, a.L = B, L
        a.sample_bb, a.sample_ang, a.sample_seq = (int(f) for f in flags)
        # Philox key in device memory (pf_sampler_args.seed_dev): a captured graph then serves every later call
        self.seed_dev = e(2, dt=torch.int64)
        a.seed_dev = self.seed_dev.data_ptr()
        # ... and the GLOBAL index of every local sample (pf_sampler_args.sample_ids, ABI 56): first_sample + b for a contiguous
        # shard (set_seed), the caller's own indices for a length bucket of a ragged batch (set_sample_ids, buckets.py)
        self.sample_ids = e(B, dt=torch.int64)
        a.sample_ids = self.sample_ids.data_ptr()
        self.args = a
        # conditioned calls (pf_sampler_*_cond): the constraint planes and the start state live in buffers THIS sampler owns, so the
        # pointers a captured graph bakes in never move; a call only rewrites their contents (set_cond)
        self.cond = bool(cond)
        if self.cond:
            self.res_flags, self.aa_allowed = e(rows, dt=torch.uint8), e(rows, dt=torch.int32)
            self.start_rot, self.start_trans, self.start_ang = e(rows, 9), e(rows, 3), e(rows, 5)
            self.start_seq = e(rows, dt=torch.int64)
            self.cargs = _capi.SamplerCondArgs()
        self.graph = None
        self.graph_k = None
        self._graph_key = None
        self._so, self._steps_done = None, 0
        self.set_seed(seed, first_sample)

    def set_seed(self, seed, first_sample=0):
        """Philox seed of the in-kernel categorical draws and the global index of this shard's first sample."""
        s = int(seed) & (2 ** 64 - 1)
        s = s - 2 ** 64 if s >= 2 ** 63 else s                          # uint64 bit pattern in an int64 tensor
        self.args.seed, self.args.first_sample = int(seed) & (2 ** 64 - 1), int(first_sample)
        self.seed_dev.copy_(torch.tensor([s, int(first_sample)], dtype=torch.int64))
        self.sample_ids.copy_(torch.arange(self.eng.B, dtype=torch.int64) + int(first_sample))

    def set_sample_ids(self, ids):
        """Global sample index of every local sample (int64 [B]) when they are not first_sample + b: keys the in-kernel Philox
        draws, so a re-ordered sub-batch draws what its samples draw in the caller's order."""
        ids = torch.as_tensor(ids, dtype=torch.int64).reshape(-1)
        assert ids.numel() == self.eng.B, (ids.numel(), self.eng.B)
        self.sample_ids.copy_(ids)

    def _launch_key(self):
        """Everything a captured graph has baked in besides device pointers that never move: the plan (pointer of block 0's pair
        input), the projection's kernel choice (active_rows hint), key-end lists on / off, caller-supplied categorical noise."""
        eng = self.eng
        key = (eng.plan_version, eng.active_rows, eng.padded, self.args.expo)
        if self.cond:                                   # which constraint planes the step kernel was launched with (NULL or the buffer)
            key += (self.cargs.res_flags, self.cargs.aa_allowed)
        return key

    def set_grid(self, grid):
        """The call's time grid (fp32 CPU tensor [num_steps], sampler.make_grid) into the device buffer the kernels and the captured
        graphs read.  EVERY call writes it: the sampler is cached, and a default call after a t_start call gets the default grid back."""
        assert grid.shape == (self.N,) and grid.dtype == torch.float32, (grid.shape, grid.dtype)
        self.ts.copy_(grid)

    def set_cond(self, cond, native):
        """The call's conditioning (sampler.make_cond, padded to the engine's length) into the owned buffers.  native = (R1, x1, ang1, seq1)
        of encode(): the start state's default, entry by entry."""
        assert self.cond, "a sampler built without cond=True has no constraint buffers"
        rows, c = self.eng.rows, self.cargs
        plane, allowed = cond.get("res_flags"), cond.get("aa_allowed")
        if plane is not None:
            self.res_flags.copy_(plane.reshape(rows))
        if allowed is not None:
            self.aa_allowed.copy_(allowed.reshape(rows))
        c.res_flags = self.res_flags.data_ptr() if plane is not None else None
        c.aa_allowed = self.aa_allowed.data_ptr() if allowed is not None else None
        c.partial = int(bool(cond["partial"]))
        if c.partial:
            for buf, key, nat, w in ((self.start_rot, "rotmats", native[0], 9), (self.start_trans, "trans", native[1], 3),
                                     (self.start_ang, "angles", native[2], 5), (self.start_seq, "seqs", native[3], 1)):
                src = cond.get(key)
                buf.copy_((nat if src is None else src).reshape(buf.shape))
        c.start_rot, c.start_trans = self.start_rot.data_ptr(), self.start_trans.data_ptr()
        c.start_ang, c.start_seq = self.start_ang.data_ptr(), self.start_seq.data_ptr()

    def set_context(self, R1, x1, ang1, seq1, gen_mask):
        rows = self.eng.rows
        self.rot1.copy_(R1.reshape(rows, 9))
        self.trans1.copy_(x1.reshape(rows, 3))
        self.ang1.copy_(ang1.reshape(rows, 5))
        self.seq1.copy_(seq1.reshape(rows))
        self.gen.copy_(gen_mask.reshape(rows).to(torch.float32))
        # the last block's tail only has to produce the generated residues' predictions (everything else is replaced by the context,
        # flow_model.py:291-311): its row tiles without one are skipped.  (DeviceSampler.SKIP_CONTEXT_ROWS = False: all rows, A/B runs)
        self.eng.want_rows(self.gen if self.SKIP_CONTEXT_ROWS else None)

    def init_state(self, noise):
        dev, rows = self.eng.device, self.eng.rows
        up = lambda k, n: noise[k].to(dev, torch.float32).reshape(rows, n).contiguous()
        rot0, tr0, ang0, sx0 = up("rot0", 9), up("trans0", 3), up("ang0", 5), up("simplex0", 20)
        if noise.get("expo") is not None:
            self.expo = noise["expo"].to(dev, torch.float32).contiguous()
            assert self.expo.shape == (2 * self.N, self.eng.B, self.eng.L, 20), self.expo.shape
            self.args.expo = self.expo.data_ptr()
        else:
            self.expo, self.args.expo = None, None
        if self.cond:
            rc = self.lib.pf_sampler_init_cond(C.byref(self.args), C.byref(self.cargs), rot0.data_ptr(), tr0.data_ptr(), ang0.data_ptr(),
                                               sx0.data_ptr(), _capi.stream_ptr())
            _capi.check(rc, "pf_sampler_init_cond")
        else:
            rc = self.lib.pf_sampler_init(C.byref(self.args), rot0.data_ptr(), tr0.data_ptr(), ang0.data_ptr(),
                                          sx0.data_ptr(), _capi.stream_ptr())
            _capi.check(rc, "pf_sampler_init")
        self._init_keep = (rot0, tr0, ang0, sx0)
        self._so = None                                # (a streamed trajectory copy belongs to ONE run from step 0; see run(stream_out=True))
        self._steps_done = 0

    def _one_step(self):
        self.eng.run(concurrent=self.CONCURRENT)
        if self.cond:
            rc = self.lib.pf_sampler_step_cond(C.byref(self.args), C.byref(self.cargs), _capi.stream_ptr())
            _capi.check(rc, "pf_sampler_step_cond")
        else:
            rc = self.lib.pf_sampler_step(C.byref(self.args), _capi.stream_ptr())
            _capi.check(rc, "pf_sampler_step")

    SKIP_CONTEXT_ROWS = True  # the last block's tail only produces the generated residues' predictions (set_context)
    CONCURRENT = False        # projection(b + 1) on a side stream beside EdgeTransition(b): measured slower (DenoiseEngine.run)
    GRAPH_STEPS = 4          # steps per replayed graph: the host-side relaunch gap (~8 us) is paid once per replay

    def _capture(self, k):
        g = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with _capi.capture_guard(), torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                for _ in range(k):
                    self._one_step()
        torch.cuda.current_stream().wait_stream(side)
        return g

    def capture(self):
        """Capture one step (network + flow update) into a hipGraph -- and GRAPH_STEPS consecutive steps into a second one:
        the step counter and the time live on the device, so every step is the same graph.  The engine runs once eagerly before
        its first capture (first-launch attribute setup must not happen under capture; the state it leaves behind is overwritten
        by init_state / the first step)."""
        if not self.eng._warm:
            self.eng.run()
        self.graph = self._capture(1)
        self.graph_k = self._capture(self.GRAPH_STEPS) if self.GRAPH_STEPS > 1 else None
        self._graph_key = self._launch_key()

    def needs_capture(self):
        return self.graph is None or self._graph_key != self._launch_key()

    STREAM_OUT_CHUNK = 32     # steps per streamed piece of the trajectory (run(stream_out=True))

    def _traj_tensors(self):
        return (self.traj_rot, self.traj_trans, self.traj_ang, self.traj_seq, self.traj_simplex)

    def _stream_chunk(self, upto):
        """Steps [copied, upto) of the five trajectory buffers -> their pinned host twins, on the copy stream, behind an event recorded
        on the compute stream HERE (the host runs ahead of the device: the event orders the copy behind the steps it copies)."""
        so = self._so
        if so is None or upto <= so["copied"]:
            return
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream())
        with torch.cuda.stream(so["stream"]):
            so["stream"].wait_event(ev)
            for h, t in zip(so["hosts"], self._traj_tensors()):
                h[so["copied"]:upto].copy_(t[so["copied"]:upto], non_blocking=True)
        so["copied"] = upto

    def run(self, n_steps=None, use_graph=True, stream_out=False):
        """stream_out: copy the trajectory to pinned host memory WHILE the loop runs (pieces of STREAM_OUT_CHUNK steps on a copy stream;
        trajectory() then only waits for the last piece): the D2H of a 200-step call of B = 64 x 128 is 280 MB = 5 ms at the PCIe rate,
        1 % of the call, otherwise spent after the loop with the device idle.  Only for a run that starts at step 0 (init_state)."""
        n = self.N if n_steps is None else n_steps
        if stream_out and self._steps_done == 0 and use_graph:
            copy_stream = getattr(self, "_copy_stream", None)
            if copy_stream is None:
                copy_stream = self._copy_stream = torch.cuda.Stream(device=self.eng.device)
            self._so = dict(stream=copy_stream, copied=0, hosts=[torch.empty(t.shape, dtype=t.dtype, pin_memory=True) for t in self._traj_tensors()])
        else:
            self._so = None
        if not use_graph:
            for _ in range(n):
                self._one_step()
            self._steps_done += n
            return
        if self.needs_capture():
            self.capture()
        k, done = self.GRAPH_STEPS, self._steps_done
        self._steps_done += n
        if self.graph_k is not None:
            for _ in range(n // k):
                self.graph_k.replay()
                done += k
                if self._so is not None and done - self._so["copied"] >= self.STREAM_OUT_CHUNK:
                    self._stream_chunk(done)
            n -= (n // k) * k
        for _ in range(n):
            self.graph.replay()
        if self._so is not None:
            self._stream_chunk(min(self._steps_done, self.N))

    def trajectory(self, pageable=False):
        """One D2H copy -> list of num_steps dicts of CPU tensors (flow_model.py:313-314,371-374).
        The tensors are VIEWS of pinned host buffers (PyTorch's caching host allocator recycles them once the views die).  A caller
        that ACCUMULATES trajectories over many complexes should pass pageable=True (FlowModel.sample(..., pageable=True)): the
        result is then copied into ordinary pageable memory and the pinned staging blocks return to the allocator at once."""
        B, L, N = self.eng.B, self.eng.L, self.N
        Lo = getattr(self, "L_out", L)                 # FlowModel.sample pads the residue axis to x16 internally: cut back

        def to_host(t):
            # pinned destination (PyTorch's caching host allocator recycles the blocks of earlier calls): the copy then runs at
            # the PCIe rate instead of the pageable-memory rate (measured 20 -> 5 ms for the 200-step trajectory of B=64 x 128)
            h = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
            h.copy_(t, non_blocking=True)
            return h
        so, self._so = getattr(self, "_so", None), None
        if so is not None and so["copied"] == N and self._steps_done == N:
            so["stream"].synchronize()                 # the whole trajectory went out while the loop ran (run(stream_out=True))
            hosts = so["hosts"]
        else:
            hosts = [to_host(t) for t in (self.traj_rot, self.traj_trans, self.traj_ang, self.traj_seq, self.traj_simplex)]   # (also BucketedSampler's gathered buffers)
        torch.cuda.current_stream().synchronize()
        if pageable:
            hosts = [torch.empty(h.shape, dtype=h.dtype).copy_(h) for h in hosts]
        rot = hosts[0].view(N, B, L, 3, 3)[:, :, :Lo]
        trans = hosts[1].view(N, B, L, 3)[:, :, :Lo]
        ang = hosts[2].view(N, B, L, 5)[:, :, :Lo]
        seq = hosts[3].view(N, B, L)[:, :, :Lo]
        sx = hosts[4].view(N, B, L, 20)[:, :, :Lo]
        R1, x1 = self.rot1.cpu().view(B, L, 3, 3)[:, :Lo], self.trans1.cpu().view(B, L, 3)[:, :Lo]
        a1, s1 = self.ang1.cpu().view(B, L, 5)[:, :Lo], self.seq1.cpu().view(B, L)[:, :Lo]
        return [{"rotmats": rot[i], "trans": trans[i], "angles": ang[i], "seqs": seq[i], "seqs_simplex": sx[i],
                 "rotmats_1": R1, "trans_1": x1, "angles_1": a1, "seqs_1": s1} for i in range(N)]
