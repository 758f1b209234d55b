"""The optimizer block of a training iteration on the device (train.py:135-146 / train_ddp.py:144-155 of the reference):

    for param in model.parameters():                       # one blocking device -> host read per parameter
        if param.grad is not None and torch.isnan(param.grad).any():
            param.grad[torch.isnan(param.grad)] = 0
    orig_grad_norm = clip_grad_norm_(model.parameters(), config.train.max_grad_norm)
    optimizer.step()

becomes `optimizer.step()` of a FusedAdam built with max_grad_norm: one call of pf_optim_step (csrc/optimizer.hip, three launches over
all parameters), no host read.  torch here = the Optimizer bookkeeping (param_groups, schedulers, state_dict) and the buffers.

Deviations from the torch block, all stated in INTEGRATION.md: a +-inf gradient entry skips the whole update (`skipped_steps`); the
gradients are read-only (NaNs are not zeroed in place, the clip is not written back); `step` lives as int32 on the device and is
exported as float32 by state_dict()."""
import ctypes as C

import numpy as np
import torch

from . import _capi

CHUNK = 4096                                              # PF_OPTIM_CHUNK of include/pepflow_hip.h
# pf_optim_tensor of include/pepflow_hip.h, 48 bytes
TENSOR_DTYPE = np.dtype([("param", "<u8"), ("grad", "<u8"), ("exp_avg_off", "<i8"), ("exp_avg_sq_off", "<i8"),
                         ("numel", "<i4"), ("group", "<i4"), ("active", "<i4"), ("pad_", "<i4")])


def build_chunks(numels, chunk=CHUNK):
    """-> int32 [n_chunks, 2] of (tensor, first element): every element of every tensor in exactly one chunk, no chunk across two
    tensors, first elements multiples of `chunk`."""
    out = []
    for t, n in enumerate(numels):
        out += [(t, first) for first in range(0, int(n), chunk)]
    return np.asarray(out, dtype=np.int32).reshape(-1, 2)


def _check_param(p, where):
    if not isinstance(p, torch.Tensor):
        raise TypeError(f"{where}: expected a torch.Tensor")
    if p.is_sparse or p.layout != torch.strided:
        raise ValueError(f"{where}: sparse tensors are not supported")
    if p.dtype != torch.float32:
        raise ValueError(f"{where}: dtype {p.dtype}; FusedAdam updates float32 tensors in place")
    if not p.is_contiguous():
        raise ValueError(f"{where}: must be contiguous")


class FusedAdam(torch.optim.Optimizer):
    """Adam (L2 weight decay) / AdamW (decoupled_weight_decay=True) with the reference's NaN guard and clip_grad_norm_(max_grad_norm)
    inside the step.  param_groups, schedulers, zero_grad() and state_dict() behave as with torch.optim.Adam; state_dict() /
    load_state_dict() round-trip with torch.optim.Adam / AdamW in both directions.

    last_grad_norm (float32, what clip_grad_norm_ returns), last_nan_count and skipped_steps (int32) are 0-dim DEVICE tensors:
    reading them is the caller's synchronisation, step() performs none."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled_weight_decay=False,
                 max_grad_norm=None, *, amsgrad=False, maximize=False):
        self._built = False
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, decoupled_weight_decay=decoupled_weight_decay,
                        amsgrad=amsgrad, maximize=maximize, foreach=None, capturable=False, differentiable=False, fused=None)
        super().__init__(params, defaults)
        self.max_grad_norm = max_grad_norm
        self._hyper_rows()                                                # validates every group
        self._params, self._group_of = [], []
        for gi, group in enumerate(self.param_groups):
            for k, p in enumerate(group["params"]):
                _check_param(p, f"param_groups[{gi}]['params'][{k}]")
                if p.numel() >= 2 ** 31:
                    raise ValueError("a parameter of 2^31 elements or more is not supported")
                self._params.append(p)
                self._group_of.append(gi)
        if not self._params:
            raise ValueError("FusedAdam got an empty parameter list")
        dev = self._params[0].device
        if any(p.device != dev for p in self._params):
            raise ValueError("all parameters must live on one device")
        self.device = dev
        numels = [p.numel() for p in self._params]
        self._offsets, used = [], 0
        for n in numels:                                                  # state slices start on 16-byte boundaries
            self._offsets.append(used)
            used += (n + 3) // 4 * 4
        self.exp_avg = torch.zeros(max(used, 4), dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(max(used, 4), dtype=torch.float32, device=dev)
        self.steps = torch.zeros(len(numels), dtype=torch.int32, device=dev)
        self._result = torch.zeros(4, dtype=torch.int32, device=dev)
        self.last_grad_norm = self._result.view(torch.float32)[0]
        self.last_nan_count = self._result[1]
        self.skipped_steps = self._result[2]
        self._chunks_host = build_chunks(numels)
        self.n_chunks = int(self._chunks_host.shape[0])
        self._chunks = torch.from_numpy(self._chunks_host.copy()).to(dev) if self.n_chunks else None
        self._work = torch.zeros(max(64 + 16 * self.n_chunks, 64) // 8, dtype=torch.float64, device=dev)
        self._table = torch.zeros(len(numels) * TENSOR_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        self._hyper = torch.zeros((1 + len(self.param_groups)) * 8, dtype=torch.float64, device=dev)
        self._table_key = self._hyper_key = None
        for i, p in enumerate(self._params):
            o, n = self._offsets[i], numels[i]
            self.state[p] = {"step": self.steps[i], "exp_avg": self.exp_avg[o:o + n].view(p.shape),
                             "exp_avg_sq": self.exp_avg_sq[o:o + n].view(p.shape)}
        self._args = None
        self._built = True

    # ------------------------------------------------------------------ torch.optim.Optimizer surface
    def add_param_group(self, param_group):
        if self._built:
            raise ValueError("FusedAdam lays its state out at construction: add_param_group() afterwards is not supported")
        super().add_param_group(param_group)

    def _hyper_rows(self):
        """-> the float64 rows of the device table, from param_groups as they are NOW (schedulers write param_groups[i]['lr'])."""
        mn = self.max_grad_norm
        rows = [[float(mn) if mn is not None else 0.0] + [0.0] * 7]
        for gi, g in enumerate(self.param_groups):
            if g.get("amsgrad") or g.get("maximize"):
                raise ValueError(f"param_groups[{gi}]: amsgrad / maximize are not supported by FusedAdam")
            for k in ("lr", "eps", "weight_decay"):
                if isinstance(g[k], torch.Tensor):
                    raise ValueError(f"param_groups[{gi}]['{k}'] is a tensor: FusedAdam takes Python numbers (no host read in step())")
            lr, (b1, b2), eps, wd = float(g["lr"]), g["betas"], float(g["eps"]), float(g["weight_decay"])
            b1, b2 = float(b1), float(b2)
            if lr < 0.0 or eps < 0.0 or wd < 0.0 or not 0.0 <= b1 < 1.0 or not 0.0 <= b2 < 1.0:
                raise ValueError(f"param_groups[{gi}]: invalid hyper-parameters lr={lr} betas={(b1, b2)} eps={eps} weight_decay={wd}")
            rows.append([lr, b1, b2, eps, wd, 1.0 if g.get("decoupled_weight_decay") else 0.0, 0.0, 0.0])
        return rows

    def _upload(self, dst, host):
        """one asynchronous copy from a pinned staging tensor (kept by the caching host allocator until the copy has run)"""
        dst.copy_(host.pin_memory(), non_blocking=True)

    def sync_groups(self):
        """Refresh the device hyper-parameter rows when param_groups (or max_grad_norm) changed since the last call."""
        rows = self._hyper_rows()
        if rows != self._hyper_key:
            self._upload(self._hyper, torch.tensor(rows, dtype=torch.float64).reshape(-1))
            self._hyper_key = rows

    def sync_pointers(self, grads=None):
        """Refresh the device tensor table when the address of a parameter or of a gradient changed (eager autograd reallocates
        gradients; a graphed step does not).  grads: one tensor or None per parameter, default `p.grad`; None = inactive in this call."""
        params = self._params
        if grads is None:
            grads = [p.grad for p in params]
        try:
            key = [p.data_ptr() for p in params], [0 if g is None else g.data_ptr() for g in grads]
        except RuntimeError:                              # (a sparse gradient has no data_ptr: name it)
            key = None
        if key is not None and key == self._table_key:
            return
        for i, (p, g) in enumerate(zip(params, grads)):
            _check_param(p, f"parameter {i}")
            if g is not None:
                _check_param(g, f"gradient of parameter {i}")
                if g.shape != p.shape or g.device != p.device:
                    raise ValueError(f"gradient of parameter {i}: shape {tuple(g.shape)} on {g.device}, parameter {tuple(p.shape)} on {p.device}")
        tab = np.zeros(len(params), dtype=TENSOR_DTYPE)
        tab["param"], tab["grad"] = key
        tab["exp_avg_off"] = tab["exp_avg_sq_off"] = self._offsets
        tab["numel"] = [p.numel() for p in params]
        tab["group"] = self._group_of
        tab["active"] = [g is not None for g in grads]
        self._upload(self._table, torch.from_numpy(tab.view(np.uint8)))
        self._table_key = key

    def launch(self):
        """pf_optim_step on the current stream with the device tables as they are (nothing else: this is what a graph captures)."""
        if self.device.type != "cuda":
            raise _capi.PepflowHipError(f"FusedAdam: parameters are on {self.device}; pepflowww_amd only runs on a ROCm GPU (no CPU fallback)")
        lib = _capi.load()
        if self._args is None:
            a = _capi.OptimArgs()
            a.tensors, a.hyper, a.chunks = self._table.data_ptr(), self._hyper.data_ptr(), self._chunks.data_ptr()
            a.exp_avg, a.exp_avg_sq, a.steps = self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(), self.steps.data_ptr()
            a.work, a.result = self._work.data_ptr(), self._result.data_ptr()
            a.n_tensors, a.n_groups, a.n_chunks = len(self._params), len(self.param_groups), self.n_chunks
            assert lib.pf_optim_work_bytes(self.n_chunks) <= self._work.numel() * 8
            self._args = a
        _capi.check(lib.pf_optim_step(C.byref(self._args), _capi.stream_ptr()), "pf_optim_step")

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self.device.type != "cuda":
            raise _capi.PepflowHipError(f"FusedAdam: parameters are on {self.device}; pepflowww_amd only runs on a ROCm GPU (no CPU fallback)")
        self.sync_groups()
        self.sync_pointers()
        self.launch()
        return loss

    def state_dict(self):
        """torch.optim.Adam's layout: per parameter `step` (float32, 0-dim), `exp_avg`, `exp_avg_sq` as tensors of their own."""
        sd = super().state_dict()
        sd["state"] = {k: {"step": s["step"].to(torch.float32), "exp_avg": s["exp_avg"].clone(), "exp_avg_sq": s["exp_avg_sq"].clone()}
                       for k, s in sd["state"].items()}
        return sd

    def load_state_dict(self, state_dict):
        """A state_dict of FusedAdam, torch.optim.Adam or torch.optim.AdamW over the same parameters (train.py:107 resumes
        ckpt['optimizer']).  The moments and counters are copied INTO the flat device buffers; a parameter without an entry (torch keeps
        none for a parameter that never had a gradient) starts from zero."""
        groups, saved = state_dict["param_groups"], state_dict["state"]
        if len(groups) != len(self.param_groups):
            raise ValueError(f"loaded state dict has {len(groups)} parameter groups, the optimizer {len(self.param_groups)}")
        for gi, (g, mine) in enumerate(zip(groups, self.param_groups)):
            if len(g["params"]) != len(mine["params"]):
                raise ValueError(f"loaded state dict's group {gi} has {len(g['params'])} parameters, the optimizer's {len(mine['params'])}")
        ids = [i for g in groups for i in g["params"]]
        for i, s in saved.items():
            if i not in ids:
                raise ValueError(f"loaded state dict has state for an unknown parameter id {i}")
            if s.get("max_exp_avg_sq") is not None:
                raise ValueError("loaded state dict comes from an amsgrad optimizer: not supported by FusedAdam")
        for g, mine in zip(groups, self.param_groups):
            for k, v in g.items():
                if k != "params":
                    mine[k] = tuple(v) if k == "betas" else v
        self._hyper_rows()
        with torch.no_grad():
            for idx, i in enumerate(ids):
                st = self.state[self._params[idx]]
                s = saved.get(i)
                if s is None:
                    st["step"].zero_(); st["exp_avg"].zero_(); st["exp_avg_sq"].zero_()
                    continue
                if tuple(s["exp_avg"].shape) != tuple(st["exp_avg"].shape):
                    raise ValueError(f"parameter {idx}: loaded exp_avg has shape {tuple(s['exp_avg'].shape)}, expected {tuple(st['exp_avg'].shape)}")
                st["exp_avg"].copy_(s["exp_avg"])
                st["exp_avg_sq"].copy_(s["exp_avg_sq"])
                step = s["step"]
                st["step"].copy_(step if isinstance(step, torch.Tensor) else torch.tensor(int(step), dtype=torch.int32))


def get_optimizer(cfg, model, max_grad_norm=None):
    """pepflow/utils/train.py:11-26 of the reference with FusedAdam: 'adam' = L2 weight decay, 'adamw' = decoupled."""
    if cfg.type == "adam":
        return FusedAdam(model.parameters(), lr=cfg.lr, weight_decay=cfg.weight_decay, betas=(cfg.beta1, cfg.beta2),
                         max_grad_norm=max_grad_norm)
    if cfg.type == "adamw":                              # (torch.optim.AdamW's default weight_decay is whatever the config says)
        return FusedAdam(model.parameters(), lr=cfg.lr, weight_decay=cfg.weight_decay, decoupled_weight_decay=True,
                         max_grad_norm=max_grad_norm)
    raise NotImplementedError("Optimizer not supported: %s" % cfg.type)
