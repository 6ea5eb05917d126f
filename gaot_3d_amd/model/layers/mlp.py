"""MLP building blocks with the reference's names and state_dict layout (src/model/layers/mlp.py:
LinearChannelMLP :308-335, ChannelMLP :227-305); every affine map runs on the HIP GEMM."""
import torch
import torch.nn as nn

from ... import functional as GF

# per-node single linears (lifting / recovery / geoembed) stay in exact-fp32 MFMA in every mode: they are HBM-bound, so
# bf16 operands would buy nothing.  The two-layer projection is fused (Mlp2Fn) in bf16 mode.
_FP32 = 0


def activation_name(fn) -> str:
    """The reference passes activations as callables (``non_linearity=F.gelu``, mlp.py:227-335,
    ``channel_mlp_non_linearity=F.gelu``, integral_transform.py:35) or builds them from a name with ``activation_fn``
    (mlp.py:27-35: "none", "swish", or any ``F.<name>``); the HIP kernels take an activation id (csrc/common.h GAOT_ACT_*).
    Accepts the callable (F.gelu, torch.tanh, nn.ELU() ... with torch's default parameters) or its name.  The fused GNO /
    projection kernels are built for erf-GELU; every other activation runs on the general per-edge / per-node path."""
    import torch.nn.functional as F
    from ...ops import ACT
    if fn is None:
        return "none"
    if isinstance(fn, str):
        name = {"swish": "silu", "identity": "none"}.get(fn.lower(), fn.lower())
    elif isinstance(fn, nn.GELU):
        name = "gelu" if getattr(fn, "approximate", "none") == "none" else "gelu_tanh"
    elif isinstance(fn, nn.Identity):
        name = "none"
    elif isinstance(fn, nn.Module):
        table = {nn.ReLU: "relu", nn.SiLU: "silu", nn.Tanh: "tanh", nn.LeakyReLU: "leaky_relu", nn.ELU: "elu",
                 nn.Sigmoid: "sigmoid", nn.Softplus: "softplus", nn.SELU: "selu", nn.ReLU6: "relu6",
                 nn.Hardswish: "hardswish", nn.Mish: "mish"}
        name = table.get(type(fn))
        defaults = {"leaky_relu": ("negative_slope", 0.01), "elu": ("alpha", 1.0)}
        if name in defaults and getattr(fn, defaults[name][0]) != defaults[name][1]:
            raise NotImplementedError(f"{fn!r}: only torch's default parameters have a HIP kernel")
        if name == "softplus" and (fn.beta != 1.0 or fn.threshold != 20.0):
            raise NotImplementedError(f"{fn!r}: only torch's default parameters have a HIP kernel")
    else:
        table = {F.gelu: "gelu", F.relu: "relu", torch.relu: "relu", F.silu: "silu", F.tanh: "tanh", torch.tanh: "tanh",
                 F.leaky_relu: "leaky_relu", F.elu: "elu", F.sigmoid: "sigmoid", torch.sigmoid: "sigmoid",
                 F.softplus: "softplus", F.selu: "selu", F.relu6: "relu6", F.hardswish: "hardswish", F.mish: "mish"}
        name = table.get(fn)
    if name is None or name not in ACT:
        raise NotImplementedError(f"activation {fn!r} has no HIP kernel (supported: {sorted(k for k in ACT if k)})")
    return name


def _jvp_fused_eligible(self, x, dxs) -> bool:
    """may ``jvp_rows`` run as one ``ops.mlp2_jvp`` launch?  Two layers with erf-GELU between them, 32 -> {64, 128, 256} -> <= 4 with
    a first bias, x and at most three tangent planes dense fp32 [N, 32] on the GPU (independent of the precision mode: the kernel is
    exact fp32)"""
    from ... import ops
    fcs = list(self.fcs)
    if len(fcs) != 2 or self.non_linearity != "gelu" or fcs[0].bias is None or not torch.is_tensor(x) or x.dim() != 2:
        return False
    ok = lambda t: t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.shape == x.shape and t.is_contiguous()
    w1, w2 = GF._w2d(fcs[0].weight), GF._w2d(fcs[1].weight)
    if not ok(x) or x.shape[1] != w1.shape[1] or w2.shape[1] != w1.shape[0] or not all(torch.is_tensor(d) and ok(d) for d in dxs):
        return False
    if any(p.dtype != torch.float32 or not p.is_cuda for p in (w1, w2, fcs[0].bias)):
        return False
    return len(dxs) <= 3 and ops.mlp2_jvp_supported(x.shape[1], w1.shape[0], w2.shape[0], len(dxs), ops.ACT["gelu"])


def _jvp_rows(self, x, dxs, fused=None, out=None):
    """Forward-mode tangents of the MLP on rows: -> (y [N, out], [dy_d [N, out] for dx_d in dxs]) with y = ``forward_rows(x)`` in
    fp32 mode (bit for bit) and dy_d the directional derivative of y along dx_d [N, C]; exact fp32 in both precision modes, no
    dropout (evaluation), nothing recorded for autograd.
    ``fused`` None: one ``ops.mlp2_jvp`` launch with the hidden layer in registers when ``_jvp_fused_eligible``, else the chain;
    True: that launch, GaotError when the module or the operands are not eligible; False: the chain.
    The chain, per layer: z = linear(x), u_d = linear(dx_d) without bias, h = act(z), v_d = act'(z) * u_d (``ops.act_bwd``), with
    precision-0 linears; rows are taken in blocks so that no hidden tensor exceeds the input's size (the rule of
    ``MAGNODecoder._project_into``).
    ``out`` = (pred_view [N, out], jac_view [N, out, len(dxs)]): the results are written there (by the fused kernel directly) and
    the returned tangents are the views jac_view[:, :, d]."""
    from ... import ops
    fcs = list(self.fcs)
    act = self.non_linearity
    n = x.shape[0]
    cout = fcs[-1].weight.shape[0]
    if out is not None:
        pv, jv = out
        if tuple(pv.shape) != (n, cout) or tuple(jv.shape) != (n, cout, len(dxs)):
            raise ops.GaotError(f"jvp_rows: out must be ([{n}, {cout}], [{n}, {cout}, {len(dxs)}]), got {tuple(pv.shape)}, {tuple(jv.shape)}")
    eligible = fused is not False and _jvp_fused_eligible(self, x, dxs)
    if fused and not eligible:
        raise ops.GaotError("jvp_rows(fused=True): the fused kernel takes a two-layer erf-GELU MLP 32 -> {64, 128, 256} -> <= 4 with a "
                            "first bias, and x and at most three tangent planes as contiguous float32 [N, 32] on the GPU")
    if eligible:
        with torch.no_grad():
            # without ``out`` the planes are laid out [T, N, out], so that every returned tangent is a dense [N, out] tensor
            dst = out if out is not None else (None, torch.empty(len(dxs), n, cout, dtype=x.dtype, device=x.device).permute(1, 2, 0))
            y, jac = ops.mlp2_jvp(x, list(dxs), GF._w2d(fcs[0].weight), fcs[0].bias, GF._w2d(fcs[1].weight), fcs[1].bias, *dst)
        return y, [jac[:, :, d] for d in range(len(dxs))]
    hid = max([fc.weight.shape[0] for fc in fcs[:-1]], default=0)
    step = max(n, 1) if hid <= x.shape[1] else max(1024, n * x.shape[1] // hid)
    with torch.no_grad():
        if out is not None:
            y, dys = out[0], [out[1][:, :, d] for d in range(len(dxs))]
        else:
            y = torch.empty(n, cout, dtype=x.dtype, device=x.device)
            dys = [torch.empty(n, cout, dtype=x.dtype, device=x.device) for _ in dxs]
        for j in range(0, n, step):
            h = x[j:j + step]
            ds = [d[j:j + step] for d in dxs]
            for i, fc in enumerate(fcs):
                last = i == len(fcs) - 1
                h, z = GF.linear_with_preact(h, fc.weight, fc.bias, act=None if last else act, precision=_FP32)
                ds = [GF.linear(d, fc.weight, None, precision=_FP32) for d in ds]
                if not last and ops.ACT[act]:
                    ds = [ops.act_bwd(z, d, ops.ACT[act]) for d in ds]
            y[j:j + step] = h
            for o, d in zip(dys, ds):
                o[j:j + step] = d
    return y, dys


def _jet2_rows(self, x, dxs, ddxs, out=None):
    """Directional 2-jets of the MLP on rows: -> (y [N, out], d1 [N, out, nd], d2 [N, out, nd]) with y = ``forward_rows(x)`` in fp32
    mode and, per direction d, d1[:, :, d] the first and d2[:, :, d] the second directional derivative of y, given the first-order
    plane dxs[d] and the second-order plane ddxs[d] of x ([N, 32] each; any number of directions >= 1, three per ``ops.mlp2_jet2``
    launch, the value stored by the first).  Exact fp32 in both precision modes, evaluation only, nothing recorded for autograd; y
    and d1 are ``jvp_rows``'s bit for bit.  Only the fused family runs -- a two-layer erf-GELU MLP 32 -> {64, 128, 256} -> <= 4 with
    a first bias on dense fp32 GPU rows; everything else raises NotImplementedError (there is no chain for second derivatives).
    ``out`` = (pred_view [N, out], d1_view [N, out, nd], d2_view [N, out, nd]; the last two with the same strides): the results are
    written there."""
    from ... import ops
    fcs = list(self.fcs)
    nd = len(dxs)
    if nd < 1 or len(ddxs) != nd:
        raise ops.GaotError(f"jet2_rows: one dx and one ddx plane per direction, at least one direction (got {nd} and {len(ddxs)})")
    plane_ok = lambda d: torch.is_tensor(d) and d.is_cuda and d.dtype == torch.float32 and d.shape == x.shape and d.is_contiguous()
    # the module and x as for the fused tangent (no planes), then the planes and the jet kernel's own family
    if not (_jvp_fused_eligible(self, x, []) and all(plane_ok(d) for d in list(dxs) + list(ddxs)) and ops.mlp2_jet2_supported(
            x.shape[1], fcs[0].weight.shape[0], fcs[1].weight.shape[0], min(nd, 3), ops.ACT["gelu"])):
        raise NotImplementedError("jet2_rows: the fused kernel takes a two-layer erf-GELU MLP 32 -> {64, 128, 256} -> <= 4 with a first "
                                  "bias, and x and the direction planes as contiguous float32 [N, 32] on the GPU")
    n, cout = x.shape[0], fcs[-1].weight.shape[0]
    with torch.no_grad():
        if out is None:
            out = (torch.empty(n, cout, dtype=x.dtype, device=x.device), torch.empty(n, cout, nd, dtype=x.dtype, device=x.device),
                   torch.empty(n, cout, nd, dtype=x.dtype, device=x.device))
        y, d1, d2 = out
        if tuple(y.shape) != (n, cout) or tuple(d1.shape) != (n, cout, nd) or tuple(d2.shape) != (n, cout, nd):
            raise ops.GaotError(f"jet2_rows: out must be ([{n}, {cout}], [{n}, {cout}, {nd}], [{n}, {cout}, {nd}]), got "
                                f"{tuple(y.shape)}, {tuple(d1.shape)}, {tuple(d2.shape)}")
        for i in range(0, nd, 3):
            ops.mlp2_jet2(x, list(dxs[i:i + 3]), list(ddxs[i:i + 3]), GF._w2d(fcs[0].weight), fcs[0].bias, GF._w2d(fcs[1].weight),
                          fcs[1].bias, y, d1[:, :, i:i + 3], d2[:, :, i:i + 3], store_y=i == 0)
    return y, d1, d2


class LinearChannelMLP(nn.Module):
    """Stack of nn.Linear parameters [layers[j] -> layers[j+1]], activation (default erf-GELU) between, none after the
    last, nn.Dropout after every layer when ``dropout`` > 0 (reference mlp.py:308-335)."""

    def __init__(self, layers, non_linearity="gelu", dropout=0.0):
        super().__init__()
        self.n_layers = len(layers) - 1
        assert self.n_layers >= 1
        self.non_linearity = activation_name(non_linearity)
        self.dropout_p = float(dropout)
        self.fcs = nn.ModuleList([nn.Linear(layers[j], layers[j + 1]) for j in range(self.n_layers)])

    def forward(self, x):
        p = self.dropout_p if self.training else 0.0
        if p == 0.0 and GF.Mlp2Fn.eligible(x, self.fcs, self.non_linearity):   # bf16 mode, C -> {64,128,256} -> <=4: fused
            return GF.Mlp2Fn.apply(x, self.fcs[0].weight, self.fcs[0].bias, self.fcs[1].weight, self.fcs[1].bias)
        for i, fc in enumerate(self.fcs):
            x = GF.linear(x, fc.weight, fc.bias, act=self.non_linearity if i < self.n_layers - 1 else None,
                          precision=_FP32)
            x = GF.dropout(x, p, self.training)
        return x

    forward_rows = forward      # [N, C] rows in, rows out (what the encoder / decoder hand over)
    jvp_rows = _jvp_rows
    jet2_rows = _jet2_rows


class ChannelMLP(nn.Module):
    """Conv1d(k=1) parameter storage ([out,in,1]) of mlp_type='channel' (reference mlp.py:227-305).  ``forward`` takes the
    reference's channels-first layout -- [C, N], [B, C, N] or [B, C, x1, x2, ...] -- and returns the same layout;
    numerically a Conv1d(k=1) is the per-node affine map, so the kernels run on row-major [N, C] and ``forward_rows`` is
    the entry point the encoder / decoder use (they hold [N, C] and the reference only transposes around this module,
    magno.py:545,575,775,796-797)."""

    def __init__(self, in_channels, out_channels=None, hidden_channels=None, n_layers=2, n_dim=2,
                 non_linearity="gelu", dropout=0.0, **kwargs):
        super().__init__()
        self.n_layers = n_layers
        self.in_channels = in_channels
        self.out_channels = in_channels if out_channels is None else out_channels
        self.hidden_channels = in_channels if hidden_channels is None else hidden_channels
        self.non_linearity = activation_name(non_linearity)
        self.dropout_p = float(dropout)
        self.fcs = nn.ModuleList()
        for i in range(n_layers):
            cin = self.in_channels if i == 0 else self.hidden_channels
            cout = self.out_channels if i == n_layers - 1 else self.hidden_channels
            self.fcs.append(nn.Conv1d(cin, cout, 1))

    def forward_rows(self, x):
        p = self.dropout_p if self.training else 0.0
        if p == 0.0 and GF.Mlp2Fn.eligible(x, self.fcs, self.non_linearity):   # bf16 mode, C -> {64,128,256} -> <=4: fused
            return GF.Mlp2Fn.apply(x, self.fcs[0].weight, self.fcs[0].bias, self.fcs[1].weight, self.fcs[1].bias)
        for i, fc in enumerate(self.fcs):
            x = GF.linear(x, fc.weight, fc.bias, act=self.non_linearity if i < self.n_layers - 1 else None,
                          precision=_FP32)
            x = GF.dropout(x, p, self.training)
        return x

    jvp_rows = _jvp_rows
    jet2_rows = _jet2_rows

    def forward(self, x):
        size = list(x.shape)
        if x.dim() == 2:                                   # unbatched Conv1d input [C, N]
            return self.forward_rows(x.transpose(0, 1)).transpose(0, 1)
        if x.dim() < 2:
            raise ValueError(f"ChannelMLP expects [C, N] or [B, C, ...], got {tuple(size)}")
        b, c = size[0], size[1]
        rows = x.reshape(b, c, -1).permute(0, 2, 1).reshape(-1, c)      # [B * N, C]
        y = self.forward_rows(rows)
        return y.view(b, -1, self.out_channels).permute(0, 2, 1).reshape(b, self.out_channels, *size[2:])


class MLP(nn.Module):
    """reference src/model/layers/mlp.py:44-72 (the small MLP of the time-conditioned norm): ``layers`` ModuleList of
    nn.Linear, activation between them, none after the last; num_layers <= 2 collapses to ONE Linear(input, output)"""

    def __init__(self, input_size: int, output_size: int, hidden_size: int, num_layers: int = 3, activation: str = "swish"):
        super().__init__()
        if num_layers <= 2:
            self.layers = nn.ModuleList([nn.Linear(input_size, output_size)])
        else:
            self.layers = nn.ModuleList([nn.Linear(input_size, hidden_size)])
            for _ in range(num_layers - 2):
                self.layers.append(nn.Linear(hidden_size, hidden_size))
            self.layers.append(nn.Linear(hidden_size, output_size))
        if activation not in ("none", "swish", "silu", "gelu", "relu"):
            raise ValueError(f"Activation function {activation} not found")
        self.activation = {"swish": "silu"}.get(activation, activation)

    def forward(self, x):
        act = None if self.activation == "none" else self.activation
        for layer in self.layers[:-1]:
            x = GF.linear(x, layer.weight, layer.bias, act=act, precision=_FP32)
        return GF.linear(x, self.layers[-1].weight, self.layers[-1].bias, precision=_FP32)


class ConditionedNorm(nn.Module):
    """time-conditioned normalisation (reference mlp.py:74-128): scale = 1 + c * mlp_scale(c), bias = c * mlp_bias(c),
    out = x * scale[:, None, :] + bias[:, None, :] with c [B, 1] and x [B, S, C]"""

    def __init__(self, input_size: int, output_size: int, hidden_size: int):
        super().__init__()
        self.mlp_scale = MLP(input_size, output_size, hidden_size, num_layers=2, activation="none")
        self.mlp_bias = MLP(input_size, output_size, hidden_size, num_layers=2, activation="none")
        for layer in list(self.mlp_scale.layers) + list(self.mlp_bias.layers):
            nn.init.normal_(layer.weight, std=0.01)

    def forward(self, c, x):
        from ... import edgeops as EO
        if c is None or not torch.is_tensor(c):
            raise TypeError("ConditionedNorm needs the condition as a [batch, 1] tensor (reference mlp.py:112-126)")
        b = x.shape[0]
        c = c.to(x.device, torch.float32).reshape(b, -1)
        if c.shape[1] != 1:
            raise ValueError("ConditionedNorm on the HIP path takes one conditioning scalar per batch element")
        cs = c.reshape(b).contiguous()
        sm1 = EO.RowScaleFn.apply(self.mlp_scale(c), cs)      # c * mlp_scale(c)   (scale - 1)
        bias = EO.RowScaleFn.apply(self.mlp_bias(c), cs)      # c * mlp_bias(c)
        outs = [EO.AffineColsFn.apply(x[i].reshape(-1, x.shape[-1]), sm1[i], bias[i]) for i in range(b)]
        y = outs[0].unsqueeze(0) if b == 1 else torch.stack(outs)
        return y.view_as(x)
