"""MI355X-native WaveGlow with the reference module API.

Drop-in for reference ``waveglow/glow.py``: same class names, constructor
signatures, attribute names (``upsample``, ``WN``, ``convinv``,
``n_remaining_channels`` ...) and ``state_dict`` keys, so checkpoints and the
reference's ``train.py`` / ``inference.py`` / ``denoiser.py`` call sites keep
working.  The math does not run through these ``nn.Module``
containers: ``forward`` / ``infer`` drive the hand-written gfx950 kernels of
``libt2s_hip.so`` through the C ABI (include/t2s_hip.h).  There is no CPU or
eager-PyTorch fallback: without the library, or off-GPU, the calls raise.

Reference lines are cited per method.
"""
import ctypes
import os
from collections import namedtuple

import torch
import torch.nn.functional as F  # noqa: F401  (kept for API parity with the reference module)

from . import _lib, sampling


class _WaveGlowLossFn(torch.autograd.Function):
    """loss = (sum z^2 / (2 sigma^2) - sum_k sum log_s_k - sum_k log_det_k) / numel(z) in one fused HIP pass
    (csrc/loss_ops.hip); d/dz = z / (sigma^2 N) comes out of the same pass, d/dlog_s = d/dlog_det = -1/N.  No eager operator
    in forward or backward: the upstream gradient (a 0-dim device tensor) is applied by t2s_scale_by_scalar."""

    @staticmethod
    def forward(ctx, sigma, n_flows, z, *rest):
        log_s = [t.detach().to(torch.float32).contiguous() for t in rest[:n_flows]]
        dets = [t.detach() for t in rest[n_flows:]]
        # the model hands out log_det_W as the n_flows elements of ONE device array (views): use it in place
        d0 = dets[0]
        if all(t.dtype == torch.float32 and t.dim() == 0 and t.untyped_storage().data_ptr() == d0.untyped_storage().data_ptr()
               and t.storage_offset() == d0.storage_offset() + k for k, t in enumerate(dets)):
            log_det = d0.as_strided((n_flows,), (1,))
        else:
            log_det = torch.stack([t.to(torch.float32).reshape(()) for t in dets])
        zc = z.detach().to(torch.float32).contiguous()
        dev = zc.device
        d_z = torch.empty_like(zc) if z.requires_grad else None
        partial = torch.empty(256 * 2, dtype=torch.float64, device=dev)
        out = torch.empty(1, dtype=torch.float32, device=dev)
        ptrs = (ctypes.c_void_p * n_flows)(*[t.data_ptr() for t in log_s])
        counts = (ctypes.c_size_t * n_flows)(*[t.numel() for t in log_s])
        _lib.call("t2s_waveglow_loss", _lib.ptr(zc), zc.numel(), ptrs, counts, n_flows, _lib.ptr(log_det), float(sigma),
                  _lib.ptr(d_z), _lib.ptr(partial), _lib.ptr(out), _lib.current_stream())
        ctx.d_z, ctx.n_flows, ctx.inv_n = d_z, n_flows, 1.0 / zc.numel()
        ctx.meta = [(t.shape, t.requires_grad) for t in rest]
        ctx.z_shape = z.shape
        return out.view(())

    @staticmethod
    def backward(ctx, g):
        g32 = g.detach().to(torch.float32).contiguous()
        st = _lib.current_stream()
        gz = None
        if ctx.d_z is not None:
            gz = torch.empty_like(ctx.d_z)
            _lib.call("t2s_scale_by_scalar", _lib.ptr(ctx.d_z), gz.numel(), _lib.ptr(g32), 1.0, _lib.ptr(gz), st)
            gz = gz.view(ctx.z_shape)
        # the constant -1/N times the upstream gradient: ONE device float, broadcast to every log_s / log_det (views, no kernel)
        neg = torch.empty(1, dtype=torch.float32, device=g32.device)
        _lib.call("t2s_scale_by_scalar", None, 1, _lib.ptr(g32), -ctx.inv_n, _lib.ptr(neg), st)
        outs = [neg.view(()).expand(shape) if need else None for shape, need in ctx.meta]
        return (None, None, gz, *outs)


class WaveGlowLoss(torch.nn.Module):
    """Reference glow.py:43-59: scalar NLL of the flow output, computed by the fused HIP kernel t2s_waveglow_loss.  Like every
    other entry point of this build it needs tensors in HBM; there is no CPU path (tests use oracle.waveglow_oracle's loss)."""

    def __init__(self, sigma=1.0):
        super().__init__()
        self.sigma = sigma

    def forward(self, model_output):
        z, log_s_list, log_det_W_list = model_output
        if not z.is_cuda:
            raise _lib.T2SError("WaveGlowLoss (MI355X build) needs tensors in HBM; there is no CPU path")
        if len(log_s_list) > 16 or len(log_s_list) != len(log_det_W_list):
            raise ValueError("WaveGlowLoss: at most 16 flows, one log_det_W per log_s")
        return _WaveGlowLossFn.apply(float(self.sigma), len(log_s_list), z, *log_s_list, *log_det_W_list)


class Invertible1x1Conv(torch.nn.Module):
    """Parameter container for the invertible 1x1 convolution (reference
    glow.py:62-80: QR-orthonormal init with det forced to +1).  The conv itself
    and log|det W| are computed by ``t2s_wg_convinv`` / ``t2s_small_logdet_inv``."""

    def __init__(self, c):
        super().__init__()
        self.conv = torch.nn.Conv1d(c, c, kernel_size=1, stride=1, padding=0, bias=False)
        W = torch.linalg.qr(torch.randn(c, c))[0]
        if torch.det(W) < 0:
            W[:, 0] = -1 * W[:, 0]
        self.conv.weight.data = W.contiguous().view(c, c, 1)

    def forward(self, z, reverse=False):
        """Reference glow.py:82-102 for callers that use the module directly (WaveGlow.forward / infer drive the same kernels
        through the engine): z [B, c, T] -> (W z, B * T * log|det W|), or with reverse=True -> W^-1 z, the inverse computed on
        first use and cached as ``W_inverse`` exactly as the reference caches it."""
        if not z.is_cuda:
            raise _lib.T2SError("Invertible1x1Conv (MI355X build) needs tensors in HBM; there is no CPU path")
        B, c, T = z.shape
        st = _lib.current_stream()
        out = z.detach().to(torch.float32).contiguous().clone()
        W = _f32c(self.conv.weight).view(c, c)
        with torch.no_grad():
            if reverse:
                if not hasattr(self, "W_inverse"):
                    Winv = torch.empty(c, c, dtype=torch.float32, device=z.device)
                    _lib.call("t2s_small_logdet_inv", _lib.ptr(W), c, 1.0, None, _lib.ptr(Winv), st)
                    self.W_inverse = Winv.view(c, c, 1)
                Wi = self.W_inverse.detach().to(torch.float32).contiguous()
                _lib.call("t2s_wg_convinv", _lib.ptr(out), _lib.ptr(Wi), B, c, 0, c, T, st)
                return out.to(z.dtype)
            log_det = torch.empty(1, dtype=torch.float32, device=z.device)
            _lib.call("t2s_small_logdet_inv", _lib.ptr(W), c, float(B * T), _lib.ptr(log_det), None, st)
            _lib.call("t2s_wg_convinv", _lib.ptr(out), _lib.ptr(W), B, c, 0, c, T, st)
            return out.to(z.dtype), log_det[0]


class WN(torch.nn.Module):
    """Parameter container for the coupling network (reference glow.py:105-152):
    weight-normed ``start``, zero-initialised ``end``, and per layer a dilated
    ``in_layers[i]``, a 1x1 ``cond_layers[i]`` and a 1x1 ``res_skip_layers[i]``."""

    def __init__(self, n_in_channels, n_mel_channels, n_layers, n_channels, kernel_size):
        super().__init__()
        assert kernel_size % 2 == 1
        assert n_channels % 2 == 0
        self.n_layers = n_layers
        self.n_channels = n_channels
        self.kernel_size = kernel_size
        self.in_layers = torch.nn.ModuleList()
        self.res_skip_layers = torch.nn.ModuleList()
        self.cond_layers = torch.nn.ModuleList()
        wn = torch.nn.utils.weight_norm
        self.start = wn(torch.nn.Conv1d(n_in_channels, n_channels, 1), name="weight")
        end = torch.nn.Conv1d(n_channels, 2 * n_in_channels, 1)
        end.weight.data.zero_()
        end.bias.data.zero_()
        self.end = end
        for i in range(n_layers):
            dilation = 2 ** i
            padding = (kernel_size * dilation - dilation) // 2
            self.in_layers.append(wn(torch.nn.Conv1d(n_channels, 2 * n_channels, kernel_size,
                                                     dilation=dilation, padding=padding), name="weight"))
            self.cond_layers.append(wn(torch.nn.Conv1d(n_mel_channels, 2 * n_channels, 1), name="weight"))
            rs = 2 * n_channels if i < n_layers - 1 else n_channels
            self.res_skip_layers.append(wn(torch.nn.Conv1d(n_channels, rs, 1), name="weight"))

    def __getstate__(self):            # the back-reference to the owning WaveGlow (a weak reference) stays out of pickles / copies
        d = self.__dict__.copy()
        d.pop("_owner", None)
        return d

    def forward(self, forward_input):
        """Reference glow.py:154-175: (audio [B, n_in, L], spect [B, n_mel * n_group, L]) -> WN.end's output [B, 2 n_in, L]
        ((b ; log_s) of the coupling).  Runs on the engine of the WaveGlow this module belongs to (forward only)."""
        ref = self.__dict__.get("_owner")
        owner = ref() if ref is not None else None
        if owner is None:
            raise _lib.T2SError("WN.forward runs on the engine of the WaveGlow it belongs to; build it through WaveGlow(...)")
        audio, spect = forward_input
        with torch.no_grad():
            return owner._eng().wn_forward(self.__dict__["_flow"], audio, spect)


def _vg(conv):
    """(v, g) of a weight-normed conv, or (weight, None) after remove_weightnorm."""
    if hasattr(conv, "weight_v"):
        return conv.weight_v, conv.weight_g
    return conv.weight, None


def _f32c(t):
    return t.detach().to(torch.float32).contiguous()


_Path = namedtuple("_Path", "start_fold boundary compose")      # which kernels a no-grad call takes: _Engine.path()

# Everything a no-grad call decides, once: the path; h16 - the operand format, False: split-bf16 (hi, lo)
# planes, True: the fp16 chain of a .half() model (fp16 planes, one-plane weights); lens - None, or infer_batch's int32 [B] columns
# per entry on the device; entry - stage -> (entry point, its arguments between the stage's own and `stream`), resolved from the
# table below; pk - the plane set (_Engine.packed or .packed16) once it is packed; melwin - (M_hi, M_lo, Fp, P, K2), the mel-window
# planes of the composed conditioning, where the call takes it.
_Plan = namedtuple("_Plan", "path h16 lens entry pk melwin")

# The entry point of every stage that has more than one: a row per stage, a column per variant -
#   split-bf16 planes | infer_batch on them | the fp16 chain | infer_batch on the fp16 chain
# None: the library has no such form.  There is no fp16 form of the folded WN.start, the flow boundary, the composed conditioning
# or the x0-rebuilding residual GEMM, so the fp16 chain is the plain path; infer_batch never takes the composed conditioning; and
# the split-bf16 gate GEMMs have no _ragged partner (only the writers of the planes they read do): infer_batch launches the plain
# ones, whereas the fp16 gate GEMM has one, which skips the column tiles behind an entry's end.
_ENTRY_POINTS = {
    "pack":         ("t2s_pack_conv_weight_table", "t2s_pack_conv_weight_table",
                     "t2s_pack_conv_weight_table_h16", "t2s_pack_conv_weight_table_h16"),
    "endfold":      ("t2s_wg_endfold_weights", "t2s_wg_endfold_weights", "t2s_wg_endfold_weights_h16", "t2s_wg_endfold_weights_h16"),
    "upsample":     ("t2s_wg_upsample_squeeze", "t2s_wg_upsample_squeeze", "t2s_wg_upsample_squeeze_h16", "t2s_wg_upsample_squeeze_h16"),
    "boundary":     ("t2s_wg_flow_boundary", "t2s_wg_flow_boundary_ragged", None, None),
    "start":        ("t2s_wg_start", "t2s_wg_start_ragged", "t2s_wg_start_h16", "t2s_wg_start_h16_ragged"),
    "start_window": ("t2s_wg_start_window", "t2s_wg_start_ragged", None, None),
    "gate":         ("t2s_wg_in_cond_gate_fold", "t2s_wg_in_cond_gate_fold",
                     "t2s_wg_in_cond_gate_fold_h16", "t2s_wg_in_cond_gate_fold_h16_ragged"),
    "gate_window":  ("t2s_wg_in_win_gate_fold", "t2s_wg_in_win_gate_fold", None, None),
    "gate_melwin":  ("t2s_wg_in_melwin_gate_fold", None, None, None),
    "res":          ("t2s_wg_res_only", "t2s_wg_res_only_ragged", "t2s_wg_res_only_h16", "t2s_wg_res_only_h16_ragged"),
    "res_start":    ("t2s_wg_res_only_start", "t2s_wg_res_only_start_ragged", None, None),
}
# The entry points that take `lengths` (the plan's lens) in front of `stream`, each with the partner whose argument list it
# extends by that one pointer.
_TAKES_LENGTHS = {
    "t2s_wg_flow_boundary_ragged": "t2s_wg_flow_boundary",
    "t2s_wg_start_ragged": "t2s_wg_start_window",       # (the window arguments always: zeros and NULLs where nothing is folded)
    "t2s_wg_res_only_ragged": "t2s_wg_res_only",
    "t2s_wg_res_only_start_ragged": "t2s_wg_res_only_start",
    "t2s_wg_start_h16_ragged": "t2s_wg_start_h16",
    "t2s_wg_in_cond_gate_fold_h16_ragged": "t2s_wg_in_cond_gate_fold_h16",
    "t2s_wg_res_only_h16_ragged": "t2s_wg_res_only_h16",
}
_START_TAKES_WINDOW = ("t2s_wg_start_window", "t2s_wg_start_ragged")   # ks, nwc and the window planes behind the X planes


def _entry_point(stage, h16, ragged=False):
    return _ENTRY_POINTS[stage][2 * bool(h16) + bool(ragged)]

# What `infer_w16 = None` does on an eligible call, decided by measurement (tools/bench_vocoder_half.py against the parent commit's
# library, profiles/infer_w16_ab.txt).  The rule: the fp16 chain is the default only if it beats the split-bf16 infer of a .half()
# model - which has the folded WN.start and the one-launch flow boundaries the fp16 chain gives up - at 1000 AND 200 frames by
# more than twice the parent's own two-run spread.  Measured at 512 channels, B = 1: 31.1 / 31.3 -> 26.2 / 27.2 ms at 1000 frames
# (spread 0.14) and 11.8 / 12.0 -> 10.5 / 11.1 ms at 200 (spread 0.24): it does, at both.
_INFER_W16_AUTO = True


class _Engine:
    """Owns the HBM-resident state of one WaveGlow: packed (hi, lo) bf16 weight
    planes and the activation workspaces, and issues the kernel sequence."""

    def __init__(self, model):
        self.m = model
        self.packed = None
        self.packed_key = None
        self.ws = {}
        self.last_path = None       # the _Path of the latest forward / infer / WN.forward
        # infer() of a .half() model on fp16 planes with one-plane weights (two MFMA products per MAC, the _h16 entry points):
        # None = automatic (_INFER_W16_AUTO where the call is eligible, see w16_eligible), False = never, True = required
        self.infer_w16 = None
        self.last_infer_w16 = False     # whether the latest infer / infer_batch ran that chain
        # infer_batch() of a .half() model on the same chain through the _h16_ragged entry points, whose GEMMs skip the column tiles
        # behind an entry's end.  Opt-in: False = never (infer_batch as infer_w16 leaves it), True = required (see
        # w16_batch_eligible; infer_w16 then governs infer only); None is reserved for "automatic" and is treated as False.
        self.infer_batch_w16 = False
        self.last_infer_batch_w16 = False       # whether the latest infer_batch ran it (last_infer_w16 is True as well then)
        self.packed16 = None           # its operands, cached beside the split-bf16 ones under the same kind of key
        self.packed16_key = None
        self._keep = []             # the current call's temporaries whose pointers went to a kernel
        self._streams = {}
        # program order across streams: a call on another stream than the engine's last one waits for it before it reads a
        # cached pack, a workspace or the engine's side streams (nothing is recorded or launched on one stream)
        self.order = _lib.StreamOrder()
        self.grad_sync = None       # distributed.GradSync: bucketed RCCL all-reduce issued from inside backward
        self.gemm_events = None     # bench.py: list of (start, end) torch.cuda.Event pairs around the gate GEMM
        self.gemm_event_stride = 1  # bench.py: time every n-th gate-GEMM launch (an event pair costs ~1.5 us of stream time)
        self._gemm_launch_no = 0

    def _enter(self, device):
        """The caller's stream, ordered behind the engine's last call.  Where the stream changed, the
        resident buffers - allocated on whichever stream first needed them - are recorded as in use on this one too.  Returns (the
        stream, whether it changed): workspace() wants both for a stream's own cache."""
        cur = self.order.enter(device)
        switched = self.order.switched
        if switched:
            _lib.record_stream((self.ws, self.packed, self.packed16, self._keep), cur)
        return cur, switched

    # ------------------------------------------------------------------ geometry
    def geom(self):
        m = self.m
        wn0 = m.WN[0]
        C, nl, ks = wn0.n_channels, wn0.n_layers, wn0.kernel_size
        n_cond = m.upsample.out_channels * m.n_group
        # halo = the largest dilated tap offset, rounded up to a whole 32-row block: the channel-last weight-gradient GEMM
        # (csrc/wgrad_cl.hip) walks whole 32-row K-blocks starting at row `halo` and shifts them by up to +-halo rows, which stays
        # inside the plane only if halo % 32 == 0 (n_layers <= 5 gives 2^(nl-1) < 32)
        halo = -(-((2 ** (nl - 1)) * (ks // 2)) // 32) * 32
        g = dict(C=C, nl=nl, ks=ks, n_cond=n_cond, Cpad=-(-C // 32) * 32, Spad=-(-n_cond // 32) * 32,
                 halo=halo, Mpad1=-(-C // 128) * 256)
        # folded WN.start: logical window columns of the widest flow, and the window chunks that hold their four column sets
        g["ncol0"] = ks * (m.n_group // 2 + 1)
        g["nwc"] = 2 if 2 * g["ncol0"] <= 32 else 4
        g["nk1"] = ks * g["Cpad"] // 32 + g["Spad"] // 32
        g["nk2"] = g["Cpad"] // 32
        return g

    def path(self, compose=True):
        """The kernel path of a no-grad call, decided here only: forward, infer and wn_forward take it once, keep it as last_path
        and hand it down.  compose = False (infer_batch): the path as if T2S_COND_COMPOSE were not set.
        start_fold: layer 0 of every flow goes through WN.start folded into its gate GEMM: the taps of the n_half audio channels
        and of the ones-channel must fit 32 columns, and C must have as many 32-channel chunks as the window has (geom()["nwc"]: 2
        or 4).  T2S_START_FOLD=0 selects the unfolded layer 0 (A/B runs, the comparison test), as composed conditioning does.
        boundary: the flow boundaries also take one launch each (t2s_wg_flow_boundary: coupling of the flow before, 1x1 convolution,
        window planes) and the layer-0 residual GEMM rebuilds x0 instead of reading X planes nobody wrote (t2s_wg_res_only_start).
        Needs the residual rows in the PAIR8 order (C % 32 == 0) and a layer that has a residual half (n_layers >= 2); both kernels
        hold n_half <= 4 audio channels, as the folded WN.end does.  T2S_FLOW_BOUNDARY=0 selects the three-kernel boundary with the
        X-plane round trip (A/B runs, the comparison test)."""
        g = self.geom()
        if g["C"] % 16:         # every no-grad gate GEMM carries WN.end folded in, which the library has for such C only
            raise _lib.T2SError("WaveGlow's forward without gradients, infer and WN.forward need n_channels %% 16 == 0, not %d" % g["C"])
        compose = self.compose_geom() if compose else None
        start_fold = (compose is None and os.environ.get("T2S_START_FOLD", "1") != "0" and g["ncol0"] <= 32
                      and g["Cpad"] // 32 >= g["nwc"])
        boundary = (start_fold and os.environ.get("T2S_FLOW_BOUNDARY", "1") != "0" and g["C"] % 32 == 0 and g["nl"] >= 2
                    and self.m.n_group // 2 <= 4)
        return _Path(start_fold, boundary, compose)

    def train_check(self):
        """What the training forward (glow_autograd.forward_train) asks of the model, checked before it allocates or launches
        anything: the transposed res/skip operand of a flow's last layer has n_channels rows per tap block (t2s_pack_transposed:
        O_pad % 32 == 0) and the gate GEMM of the backward works on whole 32-channel chunks (t2s_wg_bwd_gate_dgrad: C % 32 == 0)."""
        g = self.geom()
        if g["C"] % 32:
            raise _lib.T2SError("WaveGlow's forward with gradients (training) needs n_channels %% 32 == 0, not %d" % g["C"])

    def start_fold_on(self):
        return self.path().start_fold

    def _plan(self, h16=False, lens=None):
        """The call's _Plan, made once at the top of forward, wn_forward and _infer, before anything is packed, allocated or
        launched; every stage reads its choices from it and from nothing else, and its path becomes last_path.  The fp16 chain is
        the plain path: start -> gate GEMM with WN.end folded in -> residual GEMM -> coupling -> 1x1 convolution.  infer_batch
        (lens) never takes the composed conditioning."""
        path = self.last_path = _Path(False, False, None) if h16 else self.path(compose=lens is None)
        lengths = () if lens is None else (_lib.ptr(lens),)
        entry = {}
        for stage in _ENTRY_POINTS:
            name = _entry_point(stage, h16, lens is not None)
            entry[stage] = (name, lengths if name in _TAKES_LENGTHS else ())
        return _Plan(path, h16, lens, entry, None, None)

    def _pack(self, plan, device, force=False, flow_events=None):
        """The plan with its plane set packed (pack_weights(): cached unless forced)."""
        return plan._replace(pk=self.pack_weights(device, force=force, flow_events=flow_events, res_pair8=True,
                                                  start_fold=plan.path.start_fold, h16=plan.h16))

    def _stream(self, name, device):
        """The engine's side stream of that name on that device, made on first use."""
        key = (name, str(device))
        if key not in self._streams:
            self._streams[key] = torch.cuda.Stream(device=device)
        return self._streams[key]

    # ------------------------------------------------------------------ weights
    def pack_weights(self, device, force=True, flow_events=None, res_pair8=False, start_fold=False, h16=False):
        """res_pair8: pack the residual rows of every res/skip convolution in the 8-consecutive-channels order the folded no-grad
        path's residual GEMM wants (t2s_wg_res_only(pair8 = 1)); the training path keeps the identity order.
        start_fold: layer 0 of every flow gets the operand of the folded WN.start (A0h / A0l: the composed block, then the
        conditioning weights) and its in_layers[0] planes are NOT packed (A1h / A1l of layer 0 are stale then).
        h16: the operands of the fp16 chain, kept as `packed16` beside the split-bf16 `packed` under the same kind of key: per
        layer the in / cond and the residual effective weights as ONE fp16 plane each (computed in f32 from the fp16 parameters,
        then rounded to nearest even - no lo plane), the folded WN.end as fp16 hi / lo fragments, biases and WN.start in f32.
        That set is packed once per parameter version, never forced, and never with the folded WN.start or per-flow events."""
        assert not (h16 and (start_fold or flow_events is not None))
        res_pair8 = bool(res_pair8) and self.geom()["C"] % 32 == 0
        key = tuple(p._version for p in self.m.parameters()) + (str(device), res_pair8, start_fold)
        slot = "packed16" if h16 else "packed"
        pk = getattr(self, slot)
        if (h16 or not force) and pk is not None and getattr(self, slot + "_key") == key:
            return pk
        if pk is None or pk["device"] != device:
            pk = dict(flows=self._alloc_planes(device, h16), device=device, h16=h16)
            setattr(self, slot, pk)
        srcs = self._pack_jobs(pk, res_pair8, start_fold)
        fsrcs = self._fold_jobs(pk)
        starts = self._launch_pack(pk, start_fold, flow_events)
        setattr(self, slot + "_key", key)
        pk["res_pair8"] = res_pair8
        pk["start_fold"] = start_fold
        pk["keep"] = srcs + fsrcs + starts         # what the job tables point at, for as long as the pack is cached
        return pk

    def w16_eligible(self, batch=False):
        """(ok, why not) for the fp16 chain: infer only (not infer_batch), every WN parameter fp16, n_channels % 16 == 0 and the
        shipped library (the fp16-operand diagnostic build computes everything in fp16 planes already)."""
        if batch:
            return False, "infer_batch stays on split-bf16 planes"
        if any(p.dtype != torch.float16 for wn in self.m.WN for p in wn.parameters()):
            return False, "not every WN parameter is torch.float16 (a .half() model)"
        if self.geom()["C"] % 16:
            return False, "n_channels %% 16 != 0 (%d)" % self.geom()["C"]
        if _lib.operand_format() != 0:
            return False, "the loaded library is the fp16-operand diagnostic build"
        return True, ""

    def use_w16(self, batch=False):
        """Whether this infer / infer_batch call takes the fp16 chain; raises where infer_w16 = True cannot be honoured."""
        if self.infer_w16 is False:
            return False
        ok, why = self.w16_eligible(batch)
        if self.infer_w16 is True and not ok:
            raise _lib.T2SError("infer_w16 = True: %s" % why)
        return ok and (self.infer_w16 is True or _INFER_W16_AUTO)

    _W16_BATCH_SYMBOLS = ("t2s_wg_start_h16_ragged", "t2s_wg_in_cond_gate_fold_h16_ragged", "t2s_wg_res_only_h16_ragged")

    def w16_batch_eligible(self):
        """(ok, why not) for infer_batch on the fp16 chain: what w16_eligible asks of infer - every WN parameter fp16,
        n_channels % 16 == 0, the shipped library - and a library that exports the three _h16_ragged entry points."""
        ok, why = self.w16_eligible(batch=False)
        if not ok:
            return False, why
        lib = _lib.load()
        missing = [n for n in self._W16_BATCH_SYMBOLS if not hasattr(lib, n)]
        if missing:
            return False, "the loaded library does not export %s" % ", ".join(missing)
        return True, ""

    def use_batch_w16(self):
        """Whether this infer_batch call takes the fp16 chain (infer_batch_w16 is True; None and False: no); raises where True
        cannot be honoured.  Called before anything is packed, allocated or launched."""
        if self.infer_batch_w16 is not True:
            return False
        ok, why = self.w16_batch_eligible()
        if not ok:
            raise _lib.T2SError("infer_batch_w16 = True: %s" % why)
        return True

    def _alloc_planes(self, device, h16=False):
        """The per-flow plane set of pack_weights(), zeroed.  h16: fp16 containers, no lo planes of the convolution weights and no
        folded-WN.start operand."""
        m, g = self.m, self.geom()
        C, nl = g["C"], g["nl"]
        f32 = dict(dtype=torch.float32, device=device)
        plane = lambda *shape: torch.zeros(*shape, dtype=torch.float16 if h16 else torch.bfloat16, device=device)
        bf16_only = (lambda *shape: None) if h16 else plane
        a0 = (g["nwc"] + g["Spad"] // 32, g["Mpad1"], 32)
        flows = []
        for k in range(m.n_flows):
            n_half = m.WN[k].start.in_channels
            layers = []
            for i in range(nl):
                rows2 = 2 * C if i < nl - 1 else C
                Mpad2 = _lib.padded_rows(rows2)
                layers.append(dict(
                    A1h=plane(g["nk1"], g["Mpad1"], 32), A1l=bf16_only(g["nk1"], g["Mpad1"], 32), b1=torch.zeros(g["Mpad1"], **f32),
                    A2h=plane(g["nk2"], Mpad2, 32), A2l=bf16_only(g["nk2"], Mpad2, 32), b2=torch.zeros(Mpad2, **f32), Mpad2=Mpad2,
                    s_in=torch.empty(2 * C, **f32), s_cond=torch.empty(2 * C, **f32), s_rs=torch.empty(rows2, **f32),
                    fold_A=plane(-(-C // 128) * 8192)))
            flows.append(dict(layers=layers, n_half=n_half, bes=torch.zeros(nl, 8, **f32), w_start=torch.empty(C, n_half, **f32),
                              A0h=bf16_only(*a0), A0l=bf16_only(*a0), w_inv=None))
        return flows

    def _pack_jobs(self, pk, res_pair8, start_fold):
        """The job table of t2s_pack_conv_weight_table: all 3 * n_layers * n_flows convolutions (weight-norm + split + permute),
        rebuilt only when a source tensor moved (job_key).  Returns the f32 sources in job order."""
        m, g = self.m, self.geom()
        C, nl, ks = g["C"], g["nl"], g["ks"]
        srcs = []
        specs = []      # one list of jobs per flow
        for k, wn in enumerate(m.WN):
            fl = pk["flows"][k]
            specs.append([])
            for i in range(nl):
                ly = fl["layers"][i]
                v, gg = _vg(wn.in_layers[i])
                vc, gc = _vg(wn.cond_layers[i])
                vr, gr = _vg(wn.res_skip_layers[i])
                t = [_f32c(v), None if gg is None else _f32c(gg), _f32c(wn.in_layers[i].bias), _f32c(wn.cond_layers[i].bias),
                     _f32c(vc), None if gc is None else _f32c(gc),
                     _f32c(vr), None if gr is None else _f32c(gr), _f32c(wn.res_skip_layers[i].bias)]
                srcs += t
                # (v, g, bias, bias2, A_hi, A_lo, bias_out, O, Cin, Kt, perm, C_gate, Mpad, koff, Cin_pad)
                if i == 0 and start_fold:
                    # no in_layers[0] planes (t2s_wg_startfold_weights writes the first nwc K-chunks below); the conditioning weights
                    # follow them and their job carries the layer's bias
                    specs[k].append((t[4], t[5], t[2], t[3], fl["A0h"], fl["A0l"], ly["b1"], 2 * C, g["n_cond"], 1, 1, C,
                                     g["Mpad1"], 32 * g["nwc"], g["Spad"], ly["s_cond"]))
                else:
                    specs[k].append((t[0], t[1], t[2], t[3], ly["A1h"], ly["A1l"], ly["b1"], 2 * C, C, ks, 1, C, g["Mpad1"], 0,
                                     g["Cpad"], ly["s_in"]))
                    specs[k].append((t[4], t[5], None, None, ly["A1h"], ly["A1l"], None, 2 * C, g["n_cond"], 1, 1, C, g["Mpad1"],
                                     ks * g["Cpad"], g["Spad"], ly["s_cond"]))
                # residual rows (the first C of 2C; the last layer has none) optionally in the PERM_PAIR8 order
                p8 = res_pair8 and i < nl - 1
                specs[k].append((t[6], t[7], t[8], None, ly["A2h"], ly["A2l"], ly["b2"], t[6].size(0), C, 1, 2 if p8 else 0,
                                 C if p8 else 0, ly["Mpad2"], 0, g["Cpad"], ly["s_rs"]))
        ptr_key = tuple(0 if t is None else t.data_ptr() for t in srcs) + (res_pair8, start_fold)
        if pk.get("job_key") != ptr_key:
            rows, flow_rows, flow_jobs = [], [], []
            dp = lambda t: 0 if t is None else t.data_ptr()
            for fspecs in specs:                        # every flow's jobs are a table of their own: row_start restarts per flow
                row_start = 0
                flow_jobs.append((len(rows), len(fspecs)))
                for (v, gg, b1, b2, Ah, Al, bo, O, Cin, Kt, perm, Cg, Mpad, koff, Cin_pad, so) in fspecs:
                    rows.append([dp(v), dp(gg), dp(b1), dp(b2), dp(Ah), dp(Al), dp(bo), row_start,
                                 O, Cin, Kt, perm, Cg, Mpad, koff, Cin_pad, 0, 0, dp(so)])
                    row_start += -(-O // 16)          # the table kernel packs 16 rows per workgroup
                flow_rows.append(row_start)
            pk["jobs"] = torch.tensor(rows, dtype=torch.int64).to(pk["device"])
            pk["flow_rows"] = flow_rows
            pk["flow_jobs"] = flow_jobs        # (first job, job count) per flow
            pk["job_key"] = ptr_key
        return srcs

    def _fold_jobs(self, pk):
        """The job table of t2s_wg_endfold_weights - WN.end folded into the skip path: (W_end . W_skip_i)^T per layer, from the
        scales the pack writes - rebuilt only when a source tensor moved (fold_key).  Returns the f32 sources."""
        m, g = self.m, self.geom()
        C, nl = g["C"], g["nl"]
        fsrc = []
        for k, wn in enumerate(m.WN):
            fl = pk["flows"][k]
            w_end = _f32c(wn.end.weight)
            for i in range(nl):
                vr = _f32c(_vg(wn.res_skip_layers[i])[0])
                br = _f32c(wn.res_skip_layers[i].bias)
                r0 = C if i < nl - 1 else 0
                fsrc.append((w_end, vr, br, r0, fl["layers"][i], fl["bes"], i, 2 * fl["n_half"]))
        fkey = tuple((a.data_ptr(), b.data_ptr(), c.data_ptr()) for a, b, c, *_ in fsrc)
        if pk.get("fold_key") != fkey:
            rows = []
            for (w_end, vr, br, r0, ly, bes, i, nj) in fsrc:
                rows.append([w_end.data_ptr(), vr.data_ptr() + 4 * r0 * C, ly["s_rs"].data_ptr() + 4 * r0,
                             br.data_ptr() + 4 * r0, ly["fold_A"].data_ptr(), bes.data_ptr() + 4 * 8 * i, nj, C])
            pk["fold_jobs"] = torch.tensor(rows, dtype=torch.int64).to(pk["device"])
            pk["fold_key"] = fkey
        return [t for tup in fsrc for t in tup[:3]]

    def _launch_pack(self, pk, start_fold, flow_events):
        """One table-driven launch per flow packs its 3 * n_layers convolutions (weight-norm + split + permute), one more
        builds its folded WN.end matrices, a third its `start` weights - and with start_fold a fourth composes those with
        in_layers[0] into the first nwc K-chunks of the layer-0 operand.  The first two are the entry points of the plane set's
        operand format.  With `flow_events` (the no-grad forward) the per-flow
        work is enqueued on the caller's current stream - a side stream there - and an event per flow lets the main stream
        start flow k as soon as ITS weights are packed: the pack is HBM-bound (2.1 GB per forward), the GEMMs are not."""
        m, g = self.m, self.geom()
        C, nl, ks = g["C"], g["nl"], g["ks"]
        st = _lib.current_stream()
        jobs_ptr, fold_ptr = pk["jobs"].data_ptr(), pk["fold_jobs"].data_ptr()
        pack, endfold = _entry_point("pack", pk["h16"]), _entry_point("endfold", pk["h16"])
        starts = []
        for k, wn in enumerate(m.WN):
            fl = pk["flows"][k]
            j0, nj = pk["flow_jobs"][k]
            _lib.call(pack, _lib.c_vp(jobs_ptr + j0 * 19 * 8), nj, pk["flow_rows"][k], st)
            _lib.call(endfold, _lib.c_vp(fold_ptr + k * nl * 8 * 8), nl, C, st)
            v, gg = _vg(wn.start)
            v, gg = _f32c(v), (None if gg is None else _f32c(gg))
            starts += [v, gg]
            _lib.call("t2s_weightnorm_small", _lib.ptr(v), _lib.ptr(gg), C, fl["n_half"], _lib.ptr(fl["w_start"]), st)
            if start_fold:
                v0, g0 = _vg(wn.in_layers[0])
                v0, g0, b_start = _f32c(v0), (None if g0 is None else _f32c(g0)), _f32c(wn.start.bias)
                starts += [v0, g0, b_start]
                _lib.call("t2s_wg_startfold_weights", _lib.ptr(v0), _lib.ptr(g0), _lib.ptr(fl["w_start"]),
                          _lib.ptr(b_start), C, fl["n_half"], ks, g["Mpad1"], g["nwc"], _lib.ptr(fl["A0h"]), _lib.ptr(fl["A0l"]), st)
            fl["w_inv"] = None
            if flow_events is not None:
                ev = torch.cuda.Event()
                ev.record()
                flow_events.append(ev)
        return starts

    # ------------------------------------------------------------------ composed conditioning (inverse flow)
    def compose_geom(self):
        """(P, nlag, K2) when the conditioning path can be composed with the upsampler, else None."""
        m, g = self.m, self.geom()
        up = m.upsample
        ksz, stride, G = up.kernel_size[0], up.stride[0], m.n_group
        if os.environ.get("T2S_COND_COMPOSE") != "1":      # opt-in: see DESIGN.md section 5 for the measurements
            return None
        if ksz % stride or stride % G or ((ksz // stride) * up.in_channels) % 32 or g["C"] % 16:
            return None
        return stride // G, ksz // stride, (ksz // stride) * up.in_channels

    def compose_cond(self, device):
        """(W_cond,i . U_phi) for every layer and phase as A-operand planes, and the biases with the upsampler's bias folded in.
        Built from the packed weights, so it is keyed like them; 42 MB per layer at config.json defaults (4 GB: sized for 288 GB)."""
        if self.packed.get("compose_key") == self.packed_key:
            return
        m, g = self.m, self.geom()
        P, nlag, K2 = self.compose_geom()
        C, nl, ks = g["C"], g["nl"], g["ks"]
        up = m.upsample
        st = _lib.current_stream()
        ncols = P * K2 + 1
        Lp_u = _lib.plane_rows(ncols, 0)
        sc = g["Spad"] // 32
        bf = dict(dtype=torch.bfloat16, device=device)
        U_h, U_l = torch.zeros(1, sc, Lp_u, 32, **bf), torch.zeros(1, sc, Lp_u, 32, **bf)
        W, bias = _f32c(up.weight), _f32c(up.bias)
        _lib.call("t2s_wg_upsample_basis", _lib.ptr(W), _lib.ptr(bias), up.in_channels, up.kernel_size[0], up.stride[0],
                  m.n_group, Lp_u, 0, _lib.ptr(U_h), _lib.ptr(U_l), st)
        tmp = torch.empty(2 * C, ncols, dtype=torch.float32, device=device)
        zb = torch.zeros(g["Mpad1"], dtype=torch.float32, device=device)
        cond_off = (ks * g["Cpad"] // 32) * g["Mpad1"] * 32 * 2          # bytes: the conditioning K-chunks of the packed gate weights
        mc = K2 // 32
        for k in range(m.n_flows):
            for i in range(nl):
                ly = self.packed["flows"][k]["layers"][i]
                if "Ach" not in ly:
                    ly["Ach"] = torch.zeros(P, mc, g["Mpad1"], 32, **bf)
                    ly["Acl"] = torch.zeros(P, mc, g["Mpad1"], 32, **bf)
                    ly["b1c"] = torch.zeros(g["Mpad1"], dtype=torch.float32, device=device)
                _lib.call("t2s_conv_bias_act", _lib.c_vp(ly["A1h"].data_ptr() + cond_off), _lib.c_vp(ly["A1l"].data_ptr() + cond_off),
                          _lib.ptr(zb), _lib.ptr(U_h), _lib.ptr(U_l), None, None, _lib.ptr(tmp), 0, 1, g["n_cond"], 2 * C, 1, 1, 0,
                          ncols, Lp_u, 0, g["Mpad1"], st)
                _lib.call("t2s_wg_compose_cond", _lib.ptr(tmp), _lib.ptr(ly["b1"]), 2 * C, g["Mpad1"], P, K2, ncols,
                          _lib.ptr(ly["Ach"]), _lib.ptr(ly["Acl"]), _lib.ptr(ly["b1c"]), st)
        self._keep += [U_h, U_l, tmp, zb, W, bias]
        self.packed["compose_key"] = self.packed_key

    # ------------------------------------------------------------------ workspaces
    STREAM_SHAPES = 3       # workspaces a stream keeps resident: its first, regular and last window

    def workspace(self, B, L, device, cache=None, switched=None):
        """The activation planes of a (B, L) call.  The engine keeps ONE shape resident and reallocates (zero-filled) on every
        change.  cache (a dict owned by a stream, streaming.py): that call's workspaces live there instead, at most STREAM_SHAPES
        of them, the oldest dropped first - a stream alternates between its first, regular and last window shapes - and the
        engine's own resident shape is left alone, so what the calls around a stream allocate does not change."""
        key = (B, L, str(device))
        if cache is not None and switched is not None and switched[1]:
            _lib.record_stream(cache, switched[0])          # a stream's own workspaces, as _enter() does for the engine's: what _enter() returned
        w = (self.ws if cache is None else cache).get(key)
        if w is None:
            g = self.geom()
            Lp = _lib.plane_rows(L, g["halo"])
            bf = dict(dtype=torch.bfloat16, device=device)
            xc, sc = g["Cpad"] // 32, g["Spad"] // 32
            w = dict(Lp=Lp,
                     Xh=torch.zeros(B, xc, Lp, 32, **bf), Xl=torch.zeros(B, xc, Lp, 32, **bf),
                     Ah=torch.zeros(B, xc, Lp, 32, **bf), Al=torch.zeros(B, xc, Lp, 32, **bf),
                     Sh=torch.zeros(B, sc, Lp, 32, **bf), Sl=torch.zeros(B, sc, Lp, 32, **bf),
                     Wh=torch.zeros(B, g["nwc"], Lp, 32, **bf), Wl=torch.zeros(B, g["nwc"], Lp, 32, **bf),      # folded WN.start: window
                     z2=torch.empty(B, self.m.n_group, L, dtype=torch.float32, device=device),        # one-launch flow boundaries: the other z
                     fold_acc=torch.zeros(_lib.load().t2s_wg_gate_fold_slots(B, g["C"], L), B, 8, L, dtype=torch.float32,
                                          device=device))
            if cache is None:
                self.ws = {key: w}      # keep one shape resident
            else:
                while len(cache) >= self.STREAM_SHAPES:
                    del cache[next(iter(cache))]
                cache[key] = w
        return w

    # ------------------------------------------------------------------ stages
    def _check_inputs(self, *tensors):
        for t in tensors:
            if not t.is_cuda:
                raise _lib.T2SError("WaveGlow (MI355X build) needs CUDA/HIP tensors; got a %s tensor - there is no "
                                    "CPU fallback" % t.device)

    def _upsample(self, mel, B, L, w, plan=None):
        """plan: the no-grad call's; None (the training forward): split-bf16 planes."""
        m, g = self.m, self.geom()
        up = m.upsample
        mel32 = _f32c(mel)
        W, bias = _f32c(up.weight), _f32c(up.bias)
        name = plan.entry["upsample"][0] if plan is not None else _entry_point("upsample", False)
        _lib.call(name, _lib.ptr(mel32), _lib.ptr(W), _lib.ptr(bias), B, up.in_channels,
                  mel32.size(2), up.kernel_size[0], up.stride[0], m.n_group, L, w["Lp"], g["halo"],
                  _lib.ptr(w["Sh"]), _lib.ptr(w["Sl"]), _lib.current_stream())
        self._keep += [mel32, W, bias]

    def _boundary(self, plan, k, z_in, z_out, B, L, w, prev=None, W=None):
        """The plan's flow-boundary launch in front of flow k: prev = (flow index, log_s) applies that flow's coupling, W this
        flow's 1x1 convolution, both to z_in -> z_out; always writes flow k's window planes.  prev = W = None: the window planes
        only."""
        m, g = self.m, self.geom()
        c_off, n_rem, n_half = self._flow_geom(k)
        fold_acc = bes = b_end = log_s = None
        nslots = c_off_p = nh_p = 0
        if prev is not None:
            kp, log_s = prev
            c_off_p, _, nh_p = self._flow_geom(kp)
            fold_acc, nslots = w["fold_acc"], w["fold_acc"].size(0)
            bes = plan.pk["flows"][kp]["bes"]
            b_end = _f32c(m.WN[kp].end.bias)
            self._keep.append(b_end)
        # Stream order makes the reuse of fold_acc and of the window planes safe: this launch reads the sums of the flow before
        # ahead of flow k's layer-0 gate GEMM, which re-initialises them, and writes the window planes behind the last launch (the
        # layer-0 gate GEMM of the flow before) that read them.
        name, lengths = plan.entry["boundary"]
        _lib.call(name, _lib.ptr(z_in), _lib.ptr(z_out), _lib.ptr(fold_acc), nslots, _lib.ptr(bes), g["nl"],
                  _lib.ptr(b_end), _lib.ptr(log_s), c_off_p, nh_p, _lib.ptr(W), c_off, n_rem, n_half, B, m.n_group, L, w["Lp"],
                  g["halo"], g["ks"], g["nwc"], _lib.ptr(w["Wh"]), _lib.ptr(w["Wl"]), *lengths, _lib.current_stream())

    def _wn(self, plan, k, z, B, L, w, c_off, n_half):
        """start -> n_layers x (gate GEMM with WN.end folded in, residual GEMM) as the call's plan has it; leaves WN.end's sums in
        w['fold_acc'].  With path.boundary the caller's _boundary() has written this flow's window planes from z, and x0 is rebuilt
        by the layer-0 residual GEMM.  On the fp16 chain the lo planes of the weights are None (NULL).  The workspace planes are
        16-bit containers shared by both operand formats: every row a launch reads was written by the same call's chain, and what
        neither format writes (halo, rows past L) is zero in both.  With plan.lens every writer of the X and window planes stores
        zeros from an entry's end on, and the fp16 chain's GEMMs drop the column tiles that start at or behind it (DESIGN.md
        section 5): the acts columns of such a tile keep whatever an earlier call left there, and nothing reads them."""
        m, g = self.m, self.geom()
        C, nl, ks = g["C"], g["nl"], g["ks"]
        path, P = plan.path, _lib.ptr
        fl = plan.pk["flows"][k]
        st = _lib.current_stream()
        b_start = _f32c(m.WN[k].start.bias)
        self._keep.append(b_start)
        X, S, win, acts = ((P(w[n + "h"]), P(w[n + "l"])) for n in "XSWA")
        if not path.boundary:
            # with the folded WN.start the X planes are still written (the residual stream needs x0); the layer-0 gate GEMM reads
            # the window planes instead
            name, lengths = plan.entry["start_window" if path.start_fold else "start"]
            window = ()
            if name in _START_TAKES_WINDOW:
                window = (ks, g["nwc"], *win) if path.start_fold else (0, 0, None, None)
            _lib.call(name, P(z), P(fl["w_start"]), P(b_start), B, m.n_group, c_off, n_half, C, L, w["Lp"], g["halo"], *X,
                      *window, *lengths, st)
        gate, gate_lengths = plan.entry["gate" if plan.melwin is None else "gate_melwin"]
        gate_window = plan.entry["gate_window"][0]
        res, res_lengths = plan.entry["res"]
        res_start, res_start_lengths = plan.entry["res_start"]
        pair8 = 1 if plan.pk["res_pair8"] else 0
        dims1 = (L, w["Lp"], g["halo"], g["Mpad1"])
        for i in range(nl):
            ly = fl["layers"][i]
            # bench.py divides the sampled launch time into the FLOPs of a full-K layer: the short folded layer 0 is neither
            # counted nor timed
            full_k = not (path.start_fold and i == 0)
            timed = full_k and self.gemm_events is not None and self._gemm_launch_no % self.gemm_event_stride == 0
            if full_k:
                self._gemm_launch_no += 1
            if timed:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
            out = (*acts, P(ly["fold_A"]), P(w["fold_acc"]))
            if not full_k:
                _lib.call(gate_window, P(fl["A0h"]), P(fl["A0l"]), P(ly["b1"]), *win, *S, *out, 1, B, C, g["n_cond"], g["nwc"], *dims1, st)
            elif plan.melwin is not None:       # composed conditioning from the mel-window planes (inverse flow)
                Mh, Ml, Fp, n_phase, K2 = plan.melwin
                _lib.call(gate, P(ly["A1h"]), P(ly["A1l"]), P(ly["Ach"]), P(ly["Acl"]), P(ly["b1c"]), *X, P(Mh), P(Ml), *out,
                          1 if i == 0 else 0, B, C, K2, ks, 2 ** i, *dims1, n_phase, Fp, st)
            else:
                _lib.call(gate, P(ly["A1h"]), P(ly["A1l"]), P(ly["b1"]), *X, *S, *out,
                          1 if i == 0 else 0, B, C, g["n_cond"], ks, 2 ** i, *dims1, *gate_lengths, st)
            if timed:
                e1.record()
                self.gemm_events.append((e0, e1))
            if i == nl - 1:     # the last layer has no residual half, and its skip half lives in the fold
                continue
            weights = (P(ly["A2h"]), P(ly["A2l"]), P(ly["b2"]), *acts)
            dims2 = (B, C, L, w["Lp"], g["halo"], ly["Mpad2"])
            if path.boundary and i == 0:
                _lib.call(res_start, *weights, P(z), P(fl["w_start"]), P(b_start), m.n_group, c_off, n_half, *X, *dims2,
                          *res_start_lengths, st)
            else:
                _lib.call(res, *weights, *X, *dims2, pair8, *res_lengths, st)

    def wn_forward(self, k, audio, spect):
        """WN[k].forward((audio, spect)) (reference glow.py:154-175) on the no-grad kernels: start, n_layers x (gate GEMM with
        WN.end folded in, residual GEMM), then WN.end's output (b ; log_s) without applying the coupling."""
        self._check_inputs(audio, spect)
        dev = audio.device
        self._enter(dev)
        B, n_in, L = audio.shape
        c_off, n_rem, n_half = self._flow_geom(k)
        g = self.geom()
        if n_in != n_half or spect.size(1) != g["n_cond"] or spect.size(2) != L:
            raise ValueError("WN[%d] takes audio [B, %d, L] and spect [B, %d, L]" % (k, n_half, g["n_cond"]))
        plan = self._plan()
        self._keep = []
        plan = self._pack(plan, dev)
        w = self.workspace(B, L, dev)
        st = _lib.current_stream()
        spect32 = _f32c(spect)
        _lib.call("t2s_f32_to_planes", _lib.ptr(spect32), B, g["n_cond"], L, w["Lp"], g["halo"], _lib.ptr(w["Sh"]), _lib.ptr(w["Sl"]), st)
        z = torch.zeros(B, self.m.n_group, L, dtype=torch.float32, device=dev)
        z[:, c_off:c_off + n_half] = audio.detach().to(torch.float32)
        if plan.path.boundary:
            self._boundary(plan, k, z, None, B, L, w)
        self._wn(plan, k, z, B, L, w, c_off, n_half)
        wn_out =torch.empty(B, 2 * n_half, L, dtype=torch.float32, device=dev)
        self._end_fold(k, z, None, w["fold_acc"], wn_out, B, L, c_off, n_half, reverse=False, plan=plan)
        self._keep += [spect32, z]
        return wn_out.to(audio.dtype)

    def _end_fold(self, k, z, log_s, fold_acc, wn_out, B, L, c_off, n_half, reverse, plan=None):
        """WN.end from the sums the gate GEMMs folded it into, and flow k's coupling on z (wn_out: also WN.end's output).
        plan: the no-grad call's, whose plane set the sums were built from; None (the training forward): the split-bf16 set."""
        b_end = _f32c(self.m.WN[k].end.bias)
        self._keep.append(b_end)
        pk = self.packed if plan is None else plan.pk
        _lib.call("t2s_wg_end_fold_affine", _lib.ptr(fold_acc), fold_acc.size(0), _lib.ptr(pk["flows"][k]["bes"]),
                  self.geom()["nl"], _lib.ptr(b_end), _lib.ptr(z), _lib.ptr(log_s), _lib.ptr(wn_out), B, self.m.n_group, c_off,
                  n_half, L, 1 if reverse else 0, _lib.current_stream())

    def _end_skip(self, k, z, log_s, skip, wn_out, Lp, B, L, c_off, n_half):
        """WN.end as a convolution of the skip sum, and flow k's coupling on z: the training forward where C % 16 != 0."""
        g, wn = self.geom(), self.m.WN[k]
        w_end, b_end = _f32c(wn.end.weight), _f32c(wn.end.bias)
        self._keep += [w_end, b_end]
        _lib.call("t2s_wg_end_affine", _lib.ptr(skip), _lib.ptr(w_end), _lib.ptr(b_end), _lib.ptr(z), _lib.ptr(log_s),
                  _lib.ptr(wn_out), B, self.m.n_group, c_off, n_half, g["C"], L, Lp, g["halo"], 0, _lib.current_stream())

    def _flow_geom(self, k):
        m = self.m
        c_off = m.n_early_size * (k // m.n_early_every)
        n_rem = m.n_group - c_off
        return c_off, n_rem, n_rem // 2

    def logdet_jobs(self, Ws, log_det, inverses=None):
        """Host job table of t2s_small_logdet_inv_batch(_host): per flow W_k, where log|det W_k| goes, where W_k^-1 goes or 0, n_rem."""
        return torch.tensor([[Ws[k].data_ptr(), log_det.data_ptr() + 4 * k, 0 if inverses is None else inverses[k].data_ptr(),
                              self._flow_geom(k)[1]] for k in range(self.m.n_flows)], dtype=torch.int64)

    # ------------------------------------------------------------------ forward / infer
    def forward(self, mel, audio):
        m = self.m
        self._check_inputs(mel, audio)
        dev = audio.device
        self._enter(dev)
        B, T = audio.shape
        G = m.n_group
        L = T // G
        up = m.upsample
        if (mel.size(2) - 1) * up.stride[0] + up.kernel_size[0] < T:
            raise AssertionError("upsampled spectrogram shorter than audio (reference glow.py:216)")
        plan = self._plan()
        path = plan.path
        self._keep = []
        w = self.workspace(B, L, dev)
        # The input-side work (conditioning upsampler: compute-bound; audio squeeze; 12 log-determinants) does not depend on
        # the per-forward weight pack (HBM-bound): it runs on a second HIP stream next to the pack and joins before flow 0.
        main = torch.cuda.current_stream(dev)
        side = self._stream("side", dev)
        audio32 = _f32c(audio)
        z = torch.empty(B, G, L, dtype=torch.float32, device=dev)
        # one-launch flow boundaries read one [B, G, L] buffer and write the other: the squeezed audio goes into the one that makes
        # the caller's own tensor (never the workspace's) the last one written
        if path.boundary:
            bufs = [z, w["z2"]] if m.n_flows % 2 == 0 else [w["z2"], z]
            z = bufs[0]
        log_s_list, log_det_list = [], []
        log_det = torch.empty(m.n_flows, dtype=torch.float32, device=dev)
        Ws = [_f32c(m.convinv[k].conv.weight) for k in range(m.n_flows)]
        # B*L*logdet(W_k) of all flows in one launch (reference glow.py:100)
        use_val = m.n_flows <= 16          # the table travels as a kernel argument: no per-forward host -> device copy
        jobs = self.logdet_jobs(Ws, log_det)
        if not use_val:
            jobs = jobs.to(dev)
        self._keep += [audio32, jobs] + Ws
        side.wait_stream(main)               # inputs, the job table and earlier users of the workspace are ordered before
        with torch.cuda.stream(side):
            st2 = _lib.current_stream()
            _lib.call("t2s_wg_audio_squeeze", _lib.ptr(audio32), _lib.ptr(z), B, T, G, L, 0, st2)
            self._upsample(mel, B, L, w, plan)
            ev_inputs = torch.cuda.Event()       # flow 0 needs z and the conditioning planes; the log-determinants are only
            ev_inputs.record()                   # outputs and join at the end
            if use_val:
                _lib.call("t2s_small_logdet_inv_batch_host", ctypes.c_void_p(jobs.data_ptr()), m.n_flows, float(B * L), st2)
            else:
                _lib.call("t2s_small_logdet_inv_batch", _lib.ptr(jobs), m.n_flows, float(B * L), st2)
        # The per-forward weight pack (weight_norm recompute + split + permute, HBM-bound: 1.07 GB in, 1.07 GB out) runs flow by
        # flow on a third stream; the main stream waits for flow k's event only, so all but the first flow's share of the pack
        # runs beside the GEMMs of the flows before it.  It is not free there: without these launches the 16.36 ms step at
        # 8 x 16000 is 0.98 ms shorter (profiles/weight_prep_ceiling.txt).
        pack_s = self._stream("pack", dev)
        pack_events = []
        pack_s.wait_stream(main)
        with torch.cuda.stream(pack_s):
            plan = self._pack(plan, dev, force=True, flow_events=pack_events)
        main.wait_event(ev_inputs)
        st = _lib.current_stream()
        for k in range(m.n_flows):
            main.wait_event(pack_events[k])
            c_off, n_rem, n_half = self._flow_geom(k)
            log_s = torch.empty(B, n_half, L, dtype=torch.float32, device=dev)
            if path.boundary:
                # boundary(k): coupling of flow k - 1 (none in front of flow 0), this flow's 1x1 convolution, the window planes
                z_out = bufs[(k + 1) % 2]
                self._boundary(plan, k, z, z_out, B, L, w, prev=(k - 1, log_s_list[k - 1]) if k else None, W=Ws[k])
                z = z_out
            else:
                _lib.call("t2s_wg_convinv", _lib.ptr(z), _lib.ptr(Ws[k]), B, G, c_off, n_rem, L, st)
            self._wn(plan, k, z, B, L, w, c_off, n_half)
            if not path.boundary or k == m.n_flows - 1:     # the last coupling has no boundary behind it: in place on the current buffer
                self._end_fold(k, z, log_s, w["fold_acc"], None, B, L, c_off, n_half, reverse=False, plan=plan)
            log_s_list.append(log_s)
            log_det_list.append(log_det[k])
        main.wait_stream(side)               # log_det
        return z, log_s_list, log_det_list

    def infer(self, mel, sigma, noise, seeds=None, sigmas=None):
        return self._infer(mel, sigma, noise, None, seeds, sigmas)

    def early_flows(self):
        """The flows that re-attach early channels, in the order the inverse flow meets them (the order of ``noise``'s early draws)."""
        m = self.m
        return [k for k in reversed(range(m.n_flows)) if k % m.n_early_every == 0 and k > 0]

    def noise_slices(self, z):
        """The (final, [early draws]) views of a [B, G, L] buffer of draws, as ``_infer`` assigns a ``noise`` tuple to it."""
        m = self.m
        final = z[:, m.n_group - m.n_remaining_channels:]
        early = []
        for k in self.early_flows():
            c_off = m.n_early_size * (k // m.n_early_every)
            early.append(z[:, c_off - m.n_early_size:c_off])
        return final, early

    def infer_batch(self, mel, lengths, sigma, noise, seeds=None, sigmas=None):
        """infer() on a padded batch whose entry b is lengths[b] frames long (host int64 [B], validated by the caller): the same
        launches with every writer of the X and window planes replaced by the partner that takes the lengths, which shows each
        entry zeros past its own end as its solo run shows it past L, and one more that zeroes the audio
        tails.  Always the plain conditioning path.  With infer_batch_w16 = True the launches are those of infer's fp16 chain,
        through its partners.  Returns (audio [B, stride * frames], audio lengths int64 [B] on the device)."""
        m = self.m
        self._check_inputs(mel)
        stride = m.upsample.stride[0]
        # columns per entry, once per call: the only host -> device copy, and the array every launch that takes lengths reads
        # (through page-locked memory, so that the host does not wait for the copy: long-form synthesis runs behind it unsynchronised)
        lens = (lengths * (stride // m.n_group)).to(torch.int32).pin_memory().to(mel.device, non_blocking=True)
        audio = self._infer(mel, sigma, noise, lens, seeds, sigmas)
        B, T = audio.shape
        _lib.call("t2s_zero_rows_f32", _lib.ptr(audio), _lib.ptr(lens), B, T // m.n_group, m.n_group, _lib.current_stream())
        self._keep.append(lens)
        return audio, (lengths * stride).pin_memory().to(mel.device, non_blocking=True)

    def infer_window(self, mel, col0, k0, k1, sigma, seeds, sigmas, out, out_off, ws_cache=None):
        """_infer on ``mel``, a run of an utterance's frames that starts at column ``col0`` of its draws: the same launches, with
        the keyed draws taken at that offset (t2s_wg_noise_keyed_at) and columns [k0, k1) of the result written into
        out[:, out_off:] (t2s_wg_audio_window) in place of the whole-row unsqueeze."""
        return self._infer(mel, sigma, None, None, seeds, sigmas, window=(int(col0), int(k0), int(k1), out, int(out_off)),
                           ws_cache=ws_cache)

    def _infer(self, mel, sigma, noise, lens, seeds=None, sigmas=None, window=None, ws_cache=None):
        m = self.m
        self._check_inputs(mel)
        dev = mel.device
        entered = self._enter(dev)      # (infer_batch's lengths, uploaded ahead of this, are a tensor of that call's own)
        B, _, frames = mel.shape
        G = m.n_group
        up = m.upsample
        # reference glow.py:254-255: drop the last (kernel - stride) upsampled samples
        T = (frames - 1) * up.stride[0] + up.kernel_size[0] - (up.kernel_size[0] - up.stride[0])
        L = T // G
        # (either raises before anything is launched.)  infer_batch_w16 = True puts infer_batch on the fp16 chain whatever infer_w16
        # says, which governs infer only then; otherwise infer_batch goes through use_w16(batch=True) as it always did.
        batch = lens is not None
        batch_w16 = self.last_infer_batch_w16 = batch and self.use_batch_w16()
        h16 = self.last_infer_w16 = batch_w16 or self.use_w16(batch=batch)
        plan = self._plan(h16, lens)
        path = plan.path
        self._keep = []
        plan = self._pack(plan, dev)
        w = self.workspace(B, L, dev, ws_cache, entered)
        st = _lib.current_stream()
        # Weights are packed once here, so the conditioning path can be composed with the upsampler (K = 640 -> 320 in the gate
        # GEMM, no upsampler launch) - wherever the grid is large enough for the 256-row ping-pong tiles anyway.  Opt-in
        # (T2S_COND_COMPOSE=1): with the activations in time-major planes the phase tiles read rows 2 KB apart and the gate GEMM
        # gains 3.5 % instead of 14.7 % (1000 frames: 32.5 -> 31.7 ms; 300-400 frames lose to tile padding)
        # (256: the library's own tile-height decision)
        if path.compose is not None and _lib.load().t2s_wg_gate_tile_rows(B, self.geom()["C"], L) == 256:
            P, nlag, K2 = path.compose
            self.compose_cond(dev)
            Fp = -(-frames // 256) * 256
            key = ("melwin", B, Fp, str(dev))
            mw = self.ws.get(key)
            if mw is None:
                mw = (torch.zeros(B, K2 // 32, Fp, 32, dtype=torch.bfloat16, device=dev),
                      torch.zeros(B, K2 // 32, Fp, 32, dtype=torch.bfloat16, device=dev))
                self.ws[key] = mw
            mel32 = _f32c(mel)
            _lib.call("t2s_wg_melwin_planes", _lib.ptr(mel32), B, mel32.size(1), frames, nlag, Fp, _lib.ptr(mw[0]), _lib.ptr(mw[1]), st)
            self._keep.append(mel32)
            plan = plan._replace(melwin=(mw[0], mw[1], Fp, P, K2))
        else:
            self._upsample(mel, B, L, w, plan)
        # All Gaussian draws of glow.py:260-267,284-289 live in one [B, G, L] buffer: the final
        # n_remaining channels, and in front of them the n_early_size channels re-attached at each early flow.
        z = torch.empty(B, G, L, dtype=torch.float32, device=dev)
        n_rem_final = m.n_remaining_channels
        early_ks = self.early_flows()
        if seeds is not None:
            # keyed draws (csrc/sampling.hip): z[b] is a function of (seeds[b], channel, column) - one launch, scaled as it is stored
            if window is None:
                sampling.noise_keyed(z, seeds, sigma, sigmas)
            else:
                sampling.noise_keyed_at(z, window[0], seeds, sigma, sigmas)
            self._keep += [seeds, sigmas]
        else:
            assert window is None, "a window's draws are keyed"
            if noise is None:
                noise_final = torch.randn(B, n_rem_final, L, dtype=torch.float32, device=dev)
                noise_early = [torch.randn(B, m.n_early_size, L, dtype=torch.float32, device=dev) for _ in early_ks]
            else:
                noise_final, noise_early = noise
            z[:, G - n_rem_final:] = sigma * noise_final.to(dev, torch.float32)
            for k, ne in zip(early_ks, noise_early):
                c_off = m.n_early_size * (k // m.n_early_every)
                z[:, c_off - m.n_early_size:c_off] = sigma * ne.to(dev, torch.float32)
        for k in reversed(range(m.n_flows)):
            c_off, n_rem, n_half = self._flow_geom(k)
            fl = plan.pk["flows"][k]
            if fl["w_inv"] is None:
                Wk = _f32c(m.convinv[k].conv.weight)
                fl["w_inv"] = torch.empty(n_rem, n_rem, dtype=torch.float32, device=dev)
                _lib.call("t2s_small_logdet_inv", _lib.ptr(Wk), n_rem, 1.0, None, _lib.ptr(fl["w_inv"]), st)
                fl["_Wk"] = Wk
            if path.boundary:
                self._boundary(plan, k, z, None, B, L, w)         # the window planes only
            self._wn(plan, k, z, B, L, w, c_off, n_half)
            self._end_fold(k, z, None, w["fold_acc"], None, B, L, c_off, n_half, reverse=True, plan=plan)
            _lib.call("t2s_wg_convinv", _lib.ptr(z), _lib.ptr(fl["w_inv"]), B, G, c_off, n_rem, L, st)
        if window is not None:
            _, k0, k1, out, out_off = window
            ld = out.stride(0) if B > 1 else out.size(1)        # (one row: its stride says nothing)
            _lib.call("t2s_wg_audio_window", _lib.ptr(z), B, G, L, k0, k1, _lib.ptr(out), ld, out_off, st)
            self._keep.append(z)
            return out
        audio = torch.empty(B, L * G, dtype=torch.float32, device=dev)
        _lib.call("t2s_wg_audio_squeeze", _lib.ptr(audio), _lib.ptr(z), B, L * G, G, L, 1, st)
        return audio


class WaveGlow(torch.nn.Module):
    """Reference glow.py:178-310 API on the MI355X kernels."""

    def __init__(self, n_mel_channels, n_flows, n_group, n_early_every, n_early_size, WN_config):
        super().__init__()
        self.upsample = torch.nn.ConvTranspose1d(n_mel_channels, n_mel_channels, 1024, stride=256)
        assert n_group % 2 == 0
        self.n_flows = n_flows
        self.n_group = n_group
        self.n_early_every = n_early_every
        self.n_early_size = n_early_size
        self.WN = torch.nn.ModuleList()
        self.convinv = torch.nn.ModuleList()
        n_half = n_group // 2
        n_remaining_channels = n_group
        for k in range(n_flows):
            if k % self.n_early_every == 0 and k > 0:
                n_half = n_half - self.n_early_size // 2
                n_remaining_channels = n_remaining_channels - self.n_early_size
            self.convinv.append(Invertible1x1Conv(n_remaining_channels))
            self.WN.append(WN(n_half, n_mel_channels * n_group, **WN_config))
        self.n_remaining_channels = n_remaining_channels
        self.__dict__["_engine"] = None
        self._adopt()

    def _adopt(self):
        """WN[k].forward reaches the engine through a weak reference to its owner (kept out of the module tree)."""
        import weakref
        for k, wn_k in enumerate(self.WN):
            wn_k.__dict__["_owner"] = weakref.ref(self)
            wn_k.__dict__["_flow"] = k

    def __setstate__(self, state):
        super().__setstate__(state)
        if "_engine" not in self.__dict__:
            self.__dict__["_engine"] = None
        self._adopt()

    def _eng(self):
        if self.__dict__.get("_engine") is None:
            self.__dict__["_engine"] = _Engine(self)
        return self.__dict__["_engine"]

    def __getstate__(self):            # checkpoints pickle the module object (reference waveglow/train.py:52-60)
        d = self.__dict__.copy()
        d["_engine"] = None
        return d

    def forward(self, forward_input):
        """forward_input = (mel [B, n_mel, frames], audio [B, T]) -> (z, [log_s], [log_det_W])
        (reference glow.py:207-249)."""
        spect, audio = forward_input
        f16 = _lib.operand_format() == 1
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            if f16:
                raise _lib.T2SError("the fp16-operand diagnostic build runs the no-grad forward / infer only: gradient planes "
                                    "underflow fp16 (use the shipped library for training)")
            from .glow_autograd import waveglow_forward_with_grad
            return waveglow_forward_with_grad(self, spect, audio)
        out = self._eng().forward(spect, audio)
        if f16:
            self._refuse_overflow(out[0])
        return out

    @staticmethod
    def _refuse_overflow(t, w16=False):
        """fp16 planes only (the fp16-operand build, or the fp16 chain for .half() models: w16 = True for infer, the switch's name
        for infer_batch): a plane element beyond fp16's range (65504) became inf inside the flow and shows as a non-finite output -
        an error, not a result (split-bf16 planes have f32's exponent range and need no such check)."""
        if os.environ.get("T2S_F16_GUARD", "1") == "0":     # timing runs only: the check is a device read-back per call
            return
        if not bool(torch.isfinite(t).all()):
            switch = w16 if isinstance(w16, str) else "infer_w16"
            way_out = ("set model._eng().%s = False (split-bf16 planes)" % switch if w16
                       else "use the shipped split-bf16 library") + " for this checkpoint / input"
            raise _lib.T2SError("fp16 operand planes overflowed (|x| > 65504 somewhere in the flow): result refused; " + way_out)

    def infer(self, spect, sigma=1.0, noise=None, seed=None):
        """mel [B, n_mel, frames] -> audio [B, 256*frames] (reference glow.py:251-292).
        ``noise`` = (final [B, n_remaining, L], [early draws in the reference's order]) makes the
        Gaussian draws explicit for parity tests; by default they are drawn on the device.

        ``seed`` (an int in [0, 2^63), used for every entry; or one per entry as ``infer_batch``'s ``seeds``): the draws are keyed -
        a function of (seed, channel, column) alone, made by one kernel launch straight into the flow's buffer, whatever torch's
        generator holds.  ``infer(seed=s)`` is bit for bit ``infer(noise=draw_noise([s], L))``, and entry b of
        ``infer_batch(seeds=S)`` gets the draws of ``infer(seed=S[b])``.  With a seed ``sigma`` may be a float [B] tensor."""
        seeds, sigma, sigmas = self._keyed_args("infer", spect, sigma, noise, seed)
        with torch.no_grad():
            out = self._eng().infer(spect, sigma, noise, seeds, sigmas)
        return self._finish(out, spect)

    def infer_window(self, spect, f0, f1, sigma=1.0, seed=None, final=False, halo=None, out=None, out_offset=0, _region=None,
                     _ws=None):
        """The audio of frames [f0, f1) of an utterance whose frames 0 .. F_known - 1 are ``spect`` [B, n_mel, F_known]:
        [B, stride (f1 - f0)], what ``infer(whole mel, sigma, seed=seed)[:, stride f0 : stride f1]`` holds - without the rest of the
        mel, which may not be decoded yet (streaming.py).

        The inverse flow runs on frames [max(0, f0 - left), min(F_known, f1 + right)) only, (left, right) =
        ``streaming.vocoder_halo(self)`` - the flow's reach, (99, 96) frames at the defaults - through the launches ``infer`` issues
        for a mel of that length: the same kernels and per-column arithmetic, whichever chain ``infer`` takes for the model
        (split-bf16, or fp16 for ``.half()``, with the same overflow refusal).  The draws are the keyed ones of the window's own
        columns (``t2s_wg_noise_keyed_at``), and the kept columns go straight into the result (``t2s_wg_audio_window``).  Against
        the float64 oracle a window is as exact as the whole call; against ``infer`` it differs by float rounding only where the
        GEMMs tile the two lengths differently.

        ``seed`` is required (an int, or one per entry); there is no ``noise=``.  ``final=True`` says F_known is the utterance's
        length; without it ``f1 + right > F_known`` raises T2SError before any launch, because frames not yet known would decide
        the result.  ``halo=(l, r)`` smaller than the exact one is the caller's accuracy trade (the measured curve:
        profiles/streaming.md); larger changes nothing.  ``out`` (float32 [B, >= out_offset + stride (f1 - f0)], unit stride
        along a row): the samples are written at ``out[:, out_offset:]`` and that view is returned."""
        from . import streaming
        T2SError = _lib.T2SError
        if seed is None:
            raise T2SError("infer_window: a seed is required - a window's draws are keyed by (seed, channel, column)")
        if not torch.is_tensor(spect) or not spect.is_cuda or spect.dim() != 3:
            raise T2SError("infer_window: spect must be a [B, n_mel, F] CUDA/HIP tensor - there is no CPU fallback")
        exact = streaming.vocoder_halo(self)            # (raises where stride % n_group != 0)
        left, right = exact if halo is None else (int(halo[0]), int(halo[1]))
        if left < 0 or right < 0:
            raise ValueError("infer_window: halo must be (left, right) >= 0, got %r" % (halo,))
        B, _, F_known = spect.shape
        f0, f1 = int(f0), int(f1)
        if not 0 <= f0 < f1 <= F_known:
            raise T2SError("infer_window: need 0 <= f0 < f1 <= %d known frames, got [%d, %d)" % (F_known, f0, f1))
        if f1 + right > F_known and not final:
            raise T2SError("infer_window: frames [%d, %d) need %d frames behind them and only %d are known; pass final=True if "
                           "the utterance ends there" % (f0, f1, right, F_known))
        lo, hi = (max(0, f0 - left), min(F_known, f1 + right)) if _region is None else _region
        assert 0 <= lo <= f0 and f1 <= hi <= F_known
        stride, G = self.upsample.stride[0], self.n_group
        cols, n = stride // G, stride * (f1 - f0)
        given = out is not None
        if given:
            out_offset = int(out_offset)
            if not (torch.is_tensor(out) and out.is_cuda and out.dtype == torch.float32 and out.dim() == 2 and out.size(0) == B
                    and out.stride(1) == 1 and (B == 1 or out.stride(0) >= out.size(1)) and 0 <= out_offset
                    and out_offset + n <= out.size(1)):
                raise T2SError("infer_window: out must be a float32 CUDA/HIP tensor [%d, >= %d] with unit stride along a row"
                               % (B, int(out_offset) + n))
        else:
            out, out_offset = torch.empty(B, n, dtype=torch.float32, device=spect.device), 0
        seeds, sigma, sigmas = self._keyed_args("infer_window", spect, sigma, None, seed)
        with torch.no_grad():
            self._eng().infer_window(spect[:, :, lo:hi], lo * cols, (f0 - lo) * cols, (f1 - lo) * cols, sigma, seeds, sigmas, out,
                                     out_offset, _ws)
        res = out[:, out_offset:out_offset + n]
        fin = self._finish(res, spect)
        return res if given else fin

    def infer_stream(self, pieces, sigma=1.0, seed=None, first_frames=32, window_frames=128, halo=None):
        """A generator over ``pieces``, an iterable of (mel piece [B, n_mel, n], last) in frame order (``last`` true on the final
        one; n may be 0): yields audio pieces [B, stride f] whose concatenation is ``infer(the whole mel, sigma, seed=seed)``, of
        length exactly stride F.  The first piece holds ``first_frames`` frames and is issued once first_frames + right frames
        are known, the following ones ``window_frames`` each (``streaming.plan_windows``: every frame in exactly one window, a
        window only when the frames that decide it are known or the end is).  Each window is an ``infer_window`` call; their
        workspaces - at most three shapes: first, regular, last - stay resident for the life of the generator, and the engine's
        own resident workspace is not touched.  The weights are packed once per parameter version, as for ``infer``.
        ``seed`` is required; ``halo`` as ``infer_window`` takes it.  Arguments are checked here, before the first piece is
        asked for."""
        from . import streaming
        halo = streaming._check_stream_args(self, seed, first_frames, window_frames, halo, "infer_stream")
        return (w[0] for w in streaming.stream_windows(self, pieces, sigma, seed, first_frames, window_frames, halo))

    def _keyed_args(self, who, spect, sigma, noise, seeds):
        """(seeds int64 [B] on the device or None, sigma float, per-entry sigmas or None) of infer / infer_batch; raises before any
        launch: ValueError for bad seed or sigma values, T2SError for arguments that exclude each other."""
        T2SError = _lib.T2SError
        if seeds is None:
            if torch.is_tensor(sigma) and sigma.dim() > 0:
                raise T2SError("%s: a tensor sigma (one temperature per entry) needs seed(s)" % who)
            return None, float(sigma), None
        if noise is not None:
            raise T2SError("%s: give noise or seed(s), not both" % who)
        if not spect.is_cuda or spect.dim() != 3:
            raise T2SError("%s: spect must be a [B, n_mel, F] CUDA/HIP tensor, got %s on %s" % (who, tuple(spect.shape), spect.device))
        B = spect.size(0)
        if isinstance(seeds, int) and not isinstance(seeds, bool):
            seeds = [seeds] * B
        seeds = sampling.seeds_tensor(seeds, B, spect.device, who + ": seed(s)")
        sigma, sigmas = sampling.sigmas_tensor(sigma, B, spect.device, who + ": sigma")
        if sigmas is None and not (sigma >= 0.0 and sigma != float("inf")):
            raise ValueError("%s: sigma must be finite and >= 0, got %r" % (who, sigma))
        return seeds, sigma, sigmas

    def draw_noise(self, seeds, L, sigma=1.0):
        """The keyed draws of ``infer(seed=)`` / ``infer_batch(seeds=)`` as the tuple ``noise=`` takes: (final [B, n_remaining, L],
        [early draws in the inverse flow's order]), B = len(seeds), on the model's device - views of one [B, n_group, L] buffer filled
        by one launch, sliced the way the engine assigns a ``noise`` tuple.  L = frames * stride / n_group columns.  With the default
        sigma = 1 it is the bridge to the injected path: ``infer(spect, sigma, noise=draw_noise([s], L))`` equals
        ``infer(spect, sigma, seed=s)`` bit for bit, because the kernel stores sigma * float32(draw) as that path computes it."""
        dev = self.upsample.weight.device
        if dev.type != "cuda":
            raise _lib.T2SError("WaveGlow (MI355X build) draws on the device; the model is on %s - there is no CPU fallback" % dev)
        B = int(seeds.numel()) if torch.is_tensor(seeds) else len(seeds)
        L = int(L)
        if B < 1 or L < 1:
            raise ValueError("draw_noise: needs at least one seed and one column, got %d seeds and L = %d" % (B, L))
        seeds = sampling.seeds_tensor(seeds, B, dev, "draw_noise: seeds")
        sigma, sigmas = sampling.sigmas_tensor(sigma, B, dev, "draw_noise: sigma")
        with torch.no_grad():
            z = torch.empty(B, self.n_group, L, dtype=torch.float32, device=dev)
            sampling.noise_keyed(z, seeds, sigma, sigmas)
        return self._eng().noise_slices(z)

    def _finish(self, out, spect):
        """The ending of infer and infer_batch: refuse audio that overflowed fp16 planes (the fp16 chain - infer_batch's runs on
        its own switch, and infer's never runs there - or the diagnostic build), then the mel's dtype."""
        eng = self._eng()
        if eng.last_infer_w16:
            self._refuse_overflow(out, w16="infer_batch_w16" if eng.last_infer_batch_w16 else True)
        elif _lib.operand_format() == 1:
            self._refuse_overflow(out)
        return out.to(spect.dtype) if spect.dtype in (torch.float16, torch.bfloat16) else out

    def infer_batch(self, spect, lengths, sigma=1.0, noise=None, seeds=None):
        """Vocode a batch of mels of different lengths: ``spect`` [B, n_mel, F] padded, ``lengths`` [B] integers (host or device,
        e.g. ``Tacotron.inference_batch``'s ``output_lengths`` as returned), 1 <= lengths[b] <= F.  ``noise`` = (final
        [B, n_remaining, Lmax], [early draws]) padded to Lmax = F * stride / n_group columns, entry b using its first
        lengths[b] * stride / n_group; None: drawn on the device at the padded shape.

        Returns (audio [B, stride * F], audio_lengths int64 [B] on the device): ``audio[b, :stride * lengths[b]]`` is what
        ``infer(spect[b:b+1, :, :lengths[b]], sigma, noise sliced to entry b's columns)`` returns, up to float rounding, and the
        rest of the row is 0.  What the padding of ``spect`` and of ``noise`` holds does not reach a valid sample.  Always the plain
        conditioning path (``T2S_COND_COMPOSE`` is not read).

        ``seeds`` (one int in [0, 2^63) per entry: a sequence, or an int64 tensor on the host or the device) keys the draws: entry
        b's noise is a function of (seeds[b], channel, column) alone, made by one kernel launch, so the entry gets the draws of
        ``infer(spect[b:b+1, :, :lengths[b]], sigma, seed=seeds[b])`` whatever the batch size, its place in the batch, the padded
        length or torch's generator - without ``seeds`` (and without ``noise``) the draws depend on all four.  A wrong count or a
        negative value raises ValueError before any launch; a device tensor is used as it is, with no read-back, so its values are
        not checked.  With ``seeds``, ``sigma`` may be a float [B] tensor, one temperature per entry; ``noise`` together with
        ``seeds`` raises.

        A ``.half()`` model runs on split-bf16 planes here unless ``model._eng().infer_batch_w16 = True`` (opt-in): then the batch
        takes ``infer``'s fp16 chain, its GEMMs skip the column tiles that lie wholly behind an entry's end, and a result that
        overflowed fp16 is refused as ``infer`` refuses it, judged on the valid samples."""
        T2SError = _lib.T2SError
        if not spect.is_cuda:
            raise T2SError("WaveGlow (MI355X build) needs CUDA/HIP tensors; got a %s tensor - there is no CPU fallback" % spect.device)
        if spect.dim() != 3:
            raise T2SError("infer_batch: spect must be [B, n_mel, F], got %s" % (tuple(spect.shape),))
        B, _, F_ = spect.shape
        lens = torch.as_tensor(lengths)
        if lens.is_floating_point() or lens.is_complex() or lens.dtype == torch.bool:
            raise T2SError("infer_batch: lengths must be integers, got %s" % lens.dtype)
        lens = lens.detach().to("cpu", torch.int64)           # (one read-back when they live on the device)
        if lens.dim() != 1 or lens.numel() != B:
            raise T2SError("infer_batch: lengths has shape %s, spect holds %d mels" % (tuple(lens.shape), B))
        if B == 0 or int(lens.min()) < 1 or int(lens.max()) > F_:
            raise T2SError("infer_batch: lengths must lie in [1, %d], got %s" % (F_, lens.tolist()))
        stride, G = self.upsample.stride[0], self.n_group
        if stride % G:
            raise T2SError("infer_batch needs the upsampler's stride (%d) to be a multiple of n_group (%d)" % (stride, G))
        if noise is not None:
            Lmax = F_ * stride // G
            early = [k for k in range(self.n_flows) if k % self.n_early_every == 0 and k > 0]
            ok = isinstance(noise, (tuple, list)) and len(noise) == 2 and torch.is_tensor(noise[0]) \
                and tuple(noise[0].shape) == (B, self.n_remaining_channels, Lmax) and len(noise[1]) == len(early) \
                and all(torch.is_tensor(t) and tuple(t.shape) == (B, self.n_early_size, Lmax) for t in noise[1])
            if not ok:
                raise T2SError("infer_batch: noise must be (final [%d, %d, %d], %d early draws of [%d, %d, %d])"
                               % (B, self.n_remaining_channels, Lmax, len(early), B, self.n_early_size, Lmax))
        seeds, sigma, sigmas = self._keyed_args("infer_batch", spect, sigma, noise, seeds)
        with torch.no_grad():
            out, out_lens = self._eng().infer_batch(spect, lens, sigma, noise, seeds, sigmas)
        return self._finish(out, spect), out_lens      # (the tails are zeros by now: the valid samples decide, never what the padding held)

    @staticmethod
    def remove_weightnorm(model):
        """Fold (g, v) into plain ``weight`` tensors (reference glow.py:294-310)."""
        waveglow = model
        for wn in waveglow.WN:
            wn.start = torch.nn.utils.remove_weight_norm(wn.start)
            wn.in_layers = remove(wn.in_layers)
            wn.cond_layers = remove(wn.cond_layers)
            wn.res_skip_layers = remove(wn.res_skip_layers)
        if waveglow.__dict__.get("_engine") is not None:
            waveglow.__dict__["_engine"].packed_key = None
            waveglow.__dict__["_engine"].packed16_key = None
        return waveglow


def remove(conv_list):
    new_conv_list = torch.nn.ModuleList()
    for old_conv in conv_list:
        new_conv_list.append(torch.nn.utils.remove_weight_norm(old_conv))
    return new_conv_list
