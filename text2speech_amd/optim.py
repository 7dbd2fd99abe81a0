"""Adam with torch.optim.Adam semantics (reference waveglow/train.py:79,124; train.py:187-189,225) as ONE table-driven
kernel launch over every parameter (t2s_adam_table), instead of ~5 elementwise kernels per tensor.

State layout is torch.optim.Adam's (per parameter ``step`` / ``exp_avg`` / ``exp_avg_sq``), so an optimizer ``state_dict``
written by the reference's ``torch.optim.Adam`` (waveglow/train.py:41-50) loads here and continues with the right bias
correction, and one written here loads into ``torch.optim.Adam``.

The other two optimizer lines of the reference's Tacotron loop live here too: its learning-rate schedule (``learning_rate_decay``,
train.py:62-67,210) and the global gradient norm it logs (train.py:228-229), as ``clip_grad_norm_`` or inside ``FusedAdam.step()``
(``max_grad_norm`` / ``skip_nonfinite``): a norm pass over the same job table, then Adam with its gradient scale read from device
memory, so that a clipped step needs no host round trip.
"""
import math

import torch

from . import _lib


def learning_rate_decay(init_lr, global_step, warmup_steps=4000.0):
    """The reference's schedule (train.py:62-67): linear warm-up over `warmup_steps` steps, then init_lr * sqrt(warmup_steps / step)."""
    step = global_step + 1.0
    return init_lr * warmup_steps ** 0.5 * min(step * warmup_steps ** -1.5, step ** -0.5)


def _upload_jobs(rows, device):
    """Rows [p, g, m, v, n] -> the device array of t2s_adam_job (blk_start filled in) and its number of 1024-element blocks."""
    out, blk = [], 0
    for r in rows:
        out.append(list(r) + [blk])
        blk += -(-r[4] // 1024)
    return torch.tensor(out, dtype=torch.int64).to(device), blk


def _norm_scratch(device):
    return torch.empty(_lib.load().t2s_grad_norm_partials(), dtype=torch.float64, device=device)


_clip_table = None      # the job table of the last clip_grad_norm_ call, keyed on its gradient pointers
_clip_order = _lib.StreamOrder()       # its reduction scratch is shared by every call: program order across streams


def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False):
    """torch.nn.utils.clip_grad_norm_ (train.py:228-229) as two launches over one job table: the global L2 norm, then
    g *= min(1, max_norm / (norm + 1e-6)) in place.  Returns the norm as a 0-dim f32 DEVICE tensor; nothing is read back unless
    `error_if_nonfinite` asks for it."""
    if torch.is_tensor(parameters):
        parameters = [parameters]
    grads = [p.grad for p in parameters if p.grad is not None]
    max_norm = float(max_norm)
    if float(norm_type) != 2.0:
        raise _lib.T2SError("clip_grad_norm_ computes the L2 norm only (norm_type %r)" % (norm_type,))
    if math.isnan(max_norm) or max_norm < 0:
        raise ValueError("max_norm must be >= 0, got %r" % max_norm)
    if not grads:
        return torch.zeros(())
    for g in grads:
        if g.dtype != torch.float32 or not g.is_cuda or not g.is_contiguous():
            raise _lib.T2SError("clip_grad_norm_ needs contiguous float32 GPU gradients")
    global _clip_table
    _clip_order.enter(grads[0].device)
    key = tuple(g.data_ptr() for g in grads) + tuple(g.numel() for g in grads)
    t = _clip_table
    if t is None or t["key"] != key:
        dev = grads[0].device
        jobs, blocks = _upload_jobs([[0, g.data_ptr(), 0, 0, g.numel()] for g in grads], dev)
        t = _clip_table = dict(key=key, jobs=jobs, n=len(grads), blocks=blocks, partial=_norm_scratch(dev))
    out = torch.empty(4, dtype=torch.float32, device=grads[0].device)      # a buffer of its own: the caller keeps the returned norm
    stream = _lib.current_stream()
    _lib.call("t2s_grad_norm_table", _lib.ptr(t["jobs"]), t["n"], t["blocks"], 1.0, max_norm, _lib.ptr(t["partial"]), _lib.ptr(out),
              stream)
    if error_if_nonfinite and float(out[2]) != 0.0:
        raise RuntimeError("The total norm of order 2.0 for gradients from `parameters` is non-finite, so it cannot be clipped")
    _lib.call("t2s_grad_scale_table", _lib.ptr(t["jobs"]), t["n"], t["blocks"], _lib.ptr(out), stream)
    torch.autograd.graph.increment_version(grads)       # written through raw pointers
    return out[0]


class FusedAdam(torch.optim.Optimizer):
    """max_grad_norm: clip the global L2 norm of the gradients (all parameter groups together, times ``grad_scale``) to it BEFORE the
    update, as ``torch.nn.utils.clip_grad_norm_`` ahead of ``step()`` would; ``math.inf`` only reports the norm, which is what the
    reference does (it clips after its step, train.py:225-229).  skip_nonfinite: a step whose gradient norm is inf or NaN changes no
    parameter and no moment (alone it implies ``max_grad_norm=math.inf``).  With either, ``grad_norm`` and ``found_nonfinite`` are 0-dim
    device tensors after ``step()``, valid until the next one; nothing synchronises.  Stated limit: a skipped step still advances the
    host step counter, so the bias correction is one step ahead afterwards, and ``state_dict()`` shows that count."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=None, skip_nonfinite=False):
        if max_grad_norm is not None:
            max_grad_norm = float(max_grad_norm)
            if math.isnan(max_grad_norm) or max_grad_norm < 0:
                raise ValueError("max_grad_norm must be >= 0 (math.inf: report only), got %r" % max_grad_norm)
        elif skip_nonfinite:
            max_grad_norm = math.inf
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        super().__init__(params, defaults)
        self._tables = {}
        self._step_t = {}           # per group: one shared host tensor holding the step count (torch.optim.Adam's state layout)
        self.grad_scale = 1.0       # e.g. 1/world_size after an all-reduce(SUM)
        self.max_grad_norm = max_grad_norm
        self.skip_nonfinite = bool(skip_nonfinite)
        self._norm = None           # the job table over every group, the reduction scratch and out[4] of t2s_grad_norm_table
        self.grad_norm = None
        self.found_nonfinite = None
        # a step on another stream than the last one waits for it (moments, job tables) and for the engines that read the
        # parameters it rewrites; their next calls wait for this step
        self.order = _lib.StreamOrder(writer=True)

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._tables = {}           # the cached job tables point at the moment buffers that were just replaced
        self._step_t = {}
        for group in self.param_groups:
            group.pop("step", None)     # re-derived from the loaded per-parameter state on the next step()

    def state_dict(self):
        """torch.optim.Adam's layout with a step tensor OF ITS OWN per parameter.  Internally every parameter of a group points at
        one shared host tensor (a step costs one fill_, not one per parameter); emitted as such, `torch.optim.Adam` loading the
        dict would advance the shared counter once per parameter per step."""
        sd = super().state_dict()
        for st in sd["state"].values():
            s = st.get("step")
            if s is not None:
                st["step"] = torch.tensor(float(s.item() if torch.is_tensor(s) else s), dtype=torch.float32)
        return sd

    @staticmethod
    def _loaded_step(group, state):
        """Step count of a group: torch.optim.Adam keeps it per parameter (tensor or int)."""
        best = 0
        for p in group["params"]:
            s = state.get(p, {}).get("step")
            if s is not None:
                best = max(best, int(s.item() if torch.is_tensor(s) else s))
        return best

    def _table(self, gi, group):
        ps = [p for p in group["params"] if p.grad is not None]
        for p in ps:
            st = self.state[p]
            if "exp_avg" not in st:
                st["exp_avg"] = torch.zeros_like(p)
                st["exp_avg_sq"] = torch.zeros_like(p)
        key = tuple((p.data_ptr(), p.grad.data_ptr(), self.state[p]["exp_avg"].data_ptr(),
                     self.state[p]["exp_avg_sq"].data_ptr()) for p in ps)
        t = self._tables.get(gi)
        if t is not None and t["key"] == key:
            return t
        rows = []
        for p in ps:
            st = self.state[p]
            for x in (p, p.grad, st["exp_avg"], st["exp_avg_sq"]):
                if x.dtype != torch.float32 or not x.is_cuda or not x.is_contiguous():
                    raise _lib.T2SError("FusedAdam needs contiguous float32 GPU parameters, gradients and moments")
            rows.append([p.data_ptr(), p.grad.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), p.numel()])
        jobs, blk = _upload_jobs(rows, ps[0].device)
        t = dict(key=key, jobs=jobs, n=len(rows), blocks=blk, params=ps, rows=rows)
        self._tables[gi] = t
        return t

    def _grad_norm(self, tables):
        """One norm launch pair over the gradients of every group (the norm is global, as in torch): fills out[4] on the device."""
        key = tuple(t["key"] for t in tables)
        nt = self._norm
        if nt is None or nt["key"] != key:
            dev = tables[0]["params"][0].device
            jobs, blk = _upload_jobs([r for t in tables for r in t["rows"]], dev)
            out = nt["out"] if nt is not None else torch.zeros(4, dtype=torch.float32, device=dev)
            nt = dict(key=key, jobs=jobs, n=sum(t["n"] for t in tables), blocks=blk, out=out,
                      partial=nt["partial"] if nt is not None else _norm_scratch(dev))
            self._norm = nt
            self.grad_norm, self.found_nonfinite = out[0], out[2]
        _lib.call("t2s_grad_norm_table", _lib.ptr(nt["jobs"]), nt["n"], nt["blocks"], float(self.grad_scale), self.max_grad_norm,
                  _lib.ptr(nt["partial"]), _lib.ptr(nt["out"]), _lib.current_stream())
        return nt["out"]

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        for group in self.param_groups:
            if group["params"]:
                self.order.enter(group["params"][0].device)
                break
        active = [(gi, group) for gi, group in enumerate(self.param_groups) if any(p.grad is not None for p in group["params"])]
        tables = [self._table(gi, group) for gi, group in active]
        clip = self._grad_norm(tables) if self.max_grad_norm is not None and tables else None
        for (gi, group), t in zip(active, tables):
            if "step" not in group:
                group["step"] = self._loaded_step(group, self.state)
            if gi not in self._step_t:
                self._step_t[gi] = torch.zeros((), dtype=torch.float32)
            group["step"] += 1
            self._step_t[gi].fill_(group["step"])
            for p in t["params"]:
                self.state[p]["step"] = self._step_t[gi]
            b1, b2 = group["betas"]
            args = (_lib.ptr(t["jobs"]), t["n"], t["blocks"], float(group["lr"]), float(b1), float(b2), float(group["eps"]),
                    int(group["step"]), float(self.grad_scale), float(group["weight_decay"]))
            if clip is None:
                _lib.call("t2s_adam_table", *args, _lib.current_stream())
            else:
                _lib.call("t2s_adam_table_clip", *args, _lib.ptr(clip), int(self.skip_nonfinite), _lib.current_stream())
            # The kernel wrote the parameters through raw pointers: tell autograd / every cache keyed on tensor versions
            # (WaveGlow's packed-weight cache, glow._Engine.pack_weights) that they changed.  No kernel is launched.
            torch.autograd.graph.increment_version(t["params"])
        return loss
