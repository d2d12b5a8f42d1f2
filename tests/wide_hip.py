"""The C ABI of the 256-wide perceptron kernels (csrc/mlp.hip) for tests/test_gpu_wide_mlp_ref64.py and tools/wide_mlp_ref64_report.py: a net
on the device with its sn_mlp_desc, the four entry points into buffers the caller owns (filled with a sentinel first), and the two
measurements on float data that the tests assert and the tool tabulates."""
import ctypes as C
import types

import torch

import wide_cases as K
import wide_ref64 as R
from matrix_cases import assert_bound

SENTINEL = 7.5
BACKWARD_ENTRIES = ("k_mlp_wide4-hidden", "k_mlp_wide5-bits")


def _m():
    from sanerf_hq_amd import _lib as m
    return m


def _ok(rc):
    assert rc == 0, _m().lib().sn_last_error().decode()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptrs(ts):
    return (C.c_void_p * max(len(ts), 1))(*[t.data_ptr() for t in ts])


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class DeviceNet:
    """A net's weights on the device and its sn_mlp_desc."""

    def __init__(self, net, ws, bs, dev):
        self.net = net
        self.ws = [w.float().contiguous().to(dev) for w in ws]
        self.bs = [None if (bs is None or b is None) else b.float().contiguous().to(dev) for b in (bs or [None] * len(ws))]
        d = _m().MlpDesc()
        d.num_layers, d.activation, d.skip_mask = net.layers, int(net.leaky), sum(1 << s for s in net.skip)
        d.dims[0] = net.din
        for l, w in enumerate(self.ws):
            d.weight[l], d.dims[l + 1] = w.data_ptr(), w.shape[0]
            d.bias[l] = None if self.bs[l] is None else self.bs[l].data_ptr()
        self.desc = d

    def module(self):
        """What raymarching.mlp_forward reads of a SkipConnMLP (LeakyReLU, skip_layers) or MLP (ReLU)."""
        mod = types.SimpleNamespace(net=[types.SimpleNamespace(weight=w, bias=b) for w, b in zip(self.ws, self.bs)])
        if self.net.leaky:
            mod.skip_layers = list(self.net.skip)
        return mod


def overflow_flag():
    flag = C.c_int32(0)
    _ok(_m().lib().sn_mlp_wide_overflow(C.byref(flag)))
    return flag.value


def hip_forward(dn, x, ln=None):
    """sn_mlp_wide_forward: through raymarching.mlp_forward; a ReLU net with skip layers, which no module of the package has, through the C ABI."""
    net = dn.net
    if net.leaky or not net.skip:
        from sanerf_hq_amd import raymarching as rm
        norm = None if ln is None else types.SimpleNamespace(weight=ln[0], bias=ln[1], eps=ln[2])
        return rm.mlp_forward(x, dn.module(), norm)
    lib = _m().lib()
    need = int(lib.sn_mlp_wide_workspace_bytes(C.byref(dn.desc)))
    assert need > 0, lib.sn_last_error().decode()
    ws = torch.empty(need, dtype=torch.uint8, device=x.device)
    out = torch.full((x.shape[0], net.dout), SENTINEL, device=x.device)
    _ok(lib.sn_mlp_wide_forward(C.byref(dn.desc), _p(ln[0]) if ln else None, _p(ln[1]) if ln else None, ln[2] if ln else 0.0, _p(x), x.shape[0], _p(out),
                                _p(ws), need, _stream()))
    return out


def hip_forward_train(dn, x):
    """sn_mlp_wide_forward_train_f16x3 into the test's own buffers -> hidden (list), bits (list of int32 [M, 8]), raw."""
    lib = _m().lib()
    M, nh = x.shape[0], dn.net.layers - 1
    need = int(lib.sn_mlp_wide_workspace_bytes(C.byref(dn.desc)))
    assert need > 0, lib.sn_last_error().decode()
    ws = torch.empty(need, dtype=torch.uint8, device=x.device)
    hidden = [torch.full((M, K.WIDE), SENTINEL, device=x.device) for _ in range(nh)]
    bits = [torch.full((M, 8), 0x55555555, dtype=torch.int32, device=x.device) for _ in range(nh)]
    out = torch.full((M, dn.net.dout), SENTINEL, device=x.device)
    _ok(lib.sn_mlp_wide_forward_train_f16x3(C.byref(dn.desc), _p(x), M, _ptrs(hidden), _ptrs(bits), _p(out), _p(ws), need, _stream()))
    torch.cuda.synchronize()
    return dict(hidden=hidden, bits=bits, raw=out)


def hip_backward(dn, grad_out, entry, gates):
    """sn_mlp_wide_backward (hidden given: positive where the gate is open, 0 and negative values where it is closed) or
    sn_mlp_wide_backward_bits (the bits packed by the test) -> grad_hidden (list), grad_in."""
    lib = _m().lib()
    M, nh = grad_out.shape[0], dn.net.layers - 1
    need = int(lib.sn_mlp_wide_backward_workspace_bytes(C.byref(dn.desc)))
    assert need > 0, lib.sn_last_error().decode()
    ws = torch.empty(need, dtype=torch.uint8, device=grad_out.device)
    gh = [torch.full((M, K.WIDE), SENTINEL, device=grad_out.device) for _ in range(nh)]
    gi = torch.full((M, dn.net.din), SENTINEL, device=grad_out.device)
    if entry == BACKWARD_ENTRIES[0]:
        r = torch.arange(M)[:, None] + torch.arange(K.WIDE)[None, :]
        closed = torch.where(r % 2 == 0, 0.0, -0.5 - (r % 5).float())
        hidden = [torch.where(g, 0.25 + (r % 7).float(), closed).to(grad_out.device) for g in gates]
        _ok(lib.sn_mlp_wide_backward(C.byref(dn.desc), _p(grad_out), _ptrs(hidden), M, _p(gi), _ptrs(gh), _p(ws), need, _stream()))
    else:
        bits = [R.pack_sign_bits(g).to(grad_out.device) for g in gates]
        _ok(lib.sn_mlp_wide_backward_bits(C.byref(dn.desc), _p(grad_out), _ptrs(bits), M, _p(gi), _ptrs(gh), _p(ws), need, _stream()))
    torch.cuda.synchronize()
    return dict(grad_hidden=gh, grad_in=gi)


def _cpu(d):
    return {k: ([t.cpu() for t in v] if isinstance(v, list) else v.cpu()) for k, v in d.items()}


def float_ratios(dev, c, kind):
    """Worst |err| / bound per entry point of one float case (asserted <= 1, zero-bound elements exact)."""
    d = K.float_net(c.net, c.rows, kind)
    dn = DeviceNet(c.net, d["ws"], d["bs"], dev)
    fwd = R.chain_forward(d["x"], d["ws"], d["bs"], c.net.skip, c.net.leaky)
    what = f"{K.case_id(c)} {kind}"
    x = d["x"].to(dev)
    ratios = {"forward": assert_bound(hip_forward(dn, x).cpu(), fwd["raw"], fwd["raw_bound"], what + " forward")}
    if not c.net.skip:
        got = _cpu(hip_forward_train(dn, x))
        worst = [assert_bound(h, w, b, f"{what} hidden[{l}]") for l, (h, w, b) in enumerate(zip(got["hidden"], fwd["hidden"], fwd["hidden_bound"]))]
        ratios["forward_train"] = max(worst + [assert_bound(got["raw"], fwd["raw"], fwd["raw_bound"], what + " training forward")])
        if c.net.din <= K.WIDE:
            gates = [h > 0 for h in fwd["hidden"]]                         # the statement's own hidden outputs and bits: no branch is ambiguous
            bwd = R.chain_backward(d["grad_out"], d["ws"], gates, c.net.leaky)
            for entry in BACKWARD_ENTRIES:
                gb = _cpu(hip_backward(dn, d["grad_out"].to(dev), entry, gates))
                worst = [assert_bound(gb["grad_hidden"][l], bwd["grad_hidden"][l], bwd["grad_hidden_bound"][l], f"{what} {entry} grad_hidden[{l}]")
                         for l in range(c.net.layers - 1)]
                ratios[entry] = max(worst + [assert_bound(gb["grad_in"], bwd["grad_in"], bwd["grad_in_bound"], f"{what} {entry} grad_in")])
    return ratios


def layer_norm_ratio(dev, c):
    """LayerNorm epilogue on a case of wide_cases.layer_norm_case(): worst |err| / bound (asserted <= 1) and the output, on the CPU."""
    d = K.layer_norm_case(c)
    dn = DeviceNet(c.net, d["ws"], d["bs"], dev)
    out = hip_forward(dn, d["x"].to(dev), (d["w"].to(dev), d["b"].to(dev), d["eps"])).cpu()
    return assert_bound(out, d["want"], d["bound"], K.case_id(c) + " LayerNorm"), out, d
