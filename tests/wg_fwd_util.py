"""Helpers of the WaveGlow forward kernel tests (tests/test_waveglow_fwd_kernels_gpu.py, pinned on the CPU by
tests/test_wg_fwd_util_cpu.py): a seeded WN in float64, what oracle.waveglow_oracle.wn_forward says every layer reads and writes,
and the layouts of the folded WN.end fragments and of the gate rows.  A plain module, imported by the tests; nothing here touches
the GPU."""
import torch
import torch.nn.functional as F

from oracle import waveglow_oracle as O
from text2speech_amd import planes


# ---------------------------------------------------------------------------------------------- layouts
def _endfold_decode(fold, C):
    """fold_A -> (float64 [16, 128 ceil(C / 128)] by lane row and column, hi + lo): element (c, r) is at block c >> 5, plane hi / lo,
    lane ((c >> 2) & 3) * 16 + r, element ((c >> 4) & 1) * 4 + (c & 3)"""
    a = fold.double().cpu().view(-1, 2, 64, 8)
    c = torch.arange(a.size(0) * 32)
    out = torch.zeros(16, c.numel(), dtype=torch.float64)
    for r in range(16):
        lane = ((c >> 2) & 3) * 16 + r
        e = ((c >> 4) & 1) * 4 + (c & 3)
        out[r] = a[c >> 5, 0, lane, e] + a[c >> 5, 1, lane, e]
    return out


def _gate_row(o, C):
    """packed row of output channel o of a 2C-row gate convolution (T2S_PERM_GATE)"""
    gate = (o >= C).long()
    ch = o - gate * C
    return (ch >> 7) * 256 + ((ch >> 6) & 1) * 128 + (((ch >> 4) & 3) * 2 + gate) * 16 + (ch & 15)


def plane_round(x):
    """float64 -> the float64 value a (hi, lo) plane pair holds after planes.to_planes (through f32)"""
    hi, lo = planes.split_bf16(x.to(torch.float32))
    return hi.double() + lo.double()


# ---------------------------------------------------------------------------------------------- the seeded WN
def wn_cfg(C, n_layers, kernel_size):
    return dict(WN_config=dict(n_channels=C, n_layers=n_layers, kernel_size=kernel_size))


def wn_state(C, n_layers, kernel_size, n_half, n_cond, seed):
    """A float64 CPU state_dict of one WN.0.* with weight-norm weight_v / weight_g: directions randn, gains rand + 0.5, biases
    0.1 randn, end.weight 0.05 randn.  Weight norm makes every convolution's output variance its gain squared times the input's, so
    with unit-variance audio and spect x stays near unit variance and the gates unsaturated.  Every value is drawn in f32, so
    that the kernels (f32 parameters) and the float64 oracle start from the same numbers.
    n_cond = 0 (a gate GEMM without a conditioning half): the oracle needs a conditioning convolution, so it gets one input
    channel with a zero bias, to be fed zeros (wn_inputs) - it adds exactly nothing."""
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=gen)
    sd = {}

    def conv(name, O_, Cin, Kt, zero_bias=False):
        sd[name + ".weight_v"] = rn(O_, Cin, Kt).double()
        sd[name + ".weight_g"] = (torch.rand(O_, 1, 1, generator=gen) + 0.5).double()
        sd[name + ".bias"] = (0.1 * rn(O_)).double() * (0.0 if zero_bias else 1.0)

    conv("WN.0.start", C, n_half, 1)
    for i in range(n_layers):
        conv("WN.0.in_layers.%d" % i, 2 * C, C, kernel_size)
        conv("WN.0.cond_layers.%d" % i, 2 * C, max(n_cond, 1), 1, zero_bias=n_cond == 0)
        conv("WN.0.res_skip_layers.%d" % i, 2 * C if i < n_layers - 1 else C, C, 1)
    sd["WN.0.end.weight"] = (0.05 * rn(2 * n_half, C, 1)).double()
    sd["WN.0.end.bias"] = (0.1 * rn(2 * n_half)).double()
    return sd


def wn_inputs(B, n_half, n_cond, L, seed):
    """(audio [B, n_half, L], spect [B, max(n_cond, 1), L]) float64, unit variance, f32-representable; n_cond = 0: spect is zeros"""
    gen = torch.Generator().manual_seed(seed)
    audio = torch.randn(B, n_half, L, generator=gen).double()
    spect = torch.randn(B, max(n_cond, 1), L, generator=gen).double() * (1.0 if n_cond else 0.0)
    return audio, spect


def eff(sd, name):
    """effective (weight-normed) float64 weight of WN.0.<name>"""
    return O.effective_weight(sd, "WN.0." + name)


def skip_rows(sd, cfg, i):
    """(W_skip,i [C, C], b_skip,i [C]) float64: the skip half of res_skip_layers[i] (the whole of it in the last layer)"""
    C, nl = cfg["WN_config"]["n_channels"], cfg["WN_config"]["n_layers"]
    w, b = eff(sd, "res_skip_layers.%d" % i)[:, :, 0], sd["WN.0.res_skip_layers.%d.bias" % i]
    r0 = C if i < nl - 1 else 0
    return w[r0:r0 + C], b[r0:r0 + C]


def layer_expect(sd, cfg, audio, spect):
    """One run of the oracle's wn_forward (in the dtype it is given: float64) -> (layers, out): per layer i a dict of
        x      the layer input x_i ([B, C, L]; x_0 = WN.start's output)
        acts   acts_i = tanh * sigmoid, the oracle's own tap
        sig    sigmoid_i (recomputed here from x_i; tanh_i * sigmoid_i is asserted to be the oracle's acts_i)
        x_next x_{i+1} (the oracle's tap; x_i itself in the last layer, which has no residual half)
        F      F_i = W_end . W_skip,i [2 n_half, C] (effective weights)
        fold   F_i . acts_i [B, 2 n_half, L]
        bes    W_end . b_skip,i [2 n_half]
    and out = WN.end's output [B, 2 n_half, L]."""
    wn = cfg["WN_config"]
    C, nl, ks = wn["n_channels"], wn["n_layers"], wn["kernel_size"]
    taps = []
    out = O.wn_forward(sd, cfg, 0, audio, spect, taps=taps)
    w_end = sd["WN.0.end.weight"][:, :, 0]
    x = F.conv1d(audio, eff(sd, "start"), sd["WN.0.start.bias"])
    layers = []
    for i, (acts, x_next, _) in enumerate(taps):
        d = 2 ** i
        s = F.conv1d(x, eff(sd, "in_layers.%d" % i), sd["WN.0.in_layers.%d.bias" % i], dilation=d, padding=(ks * d - d) // 2) + \
            F.conv1d(spect, eff(sd, "cond_layers.%d" % i), sd["WN.0.cond_layers.%d.bias" % i])
        sig = torch.sigmoid(s[:, C:])
        assert float((torch.tanh(s[:, :C]) * sig - acts).abs().max()) <= 1e-12 * max(1.0, float(acts.abs().max())), i
        w_skip, b_skip = skip_rows(sd, cfg, i)
        Fi = w_end @ w_skip
        layers.append(dict(x=x, acts=acts, sig=sig, x_next=x_next, F=Fi, fold=torch.einsum("jc,bct->bjt", Fi, acts),
                           bes=w_end @ b_skip))
        x = x_next
    return layers, out
