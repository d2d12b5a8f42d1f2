"""CPU: sn_adam_step_multi (one launch for every parameter tensor of the model) as far as it goes without a GPU -- the symbol, the layout
of its records, every host-side argument check (all of them run before anything touches the device), the constructor of
optim.Adam(multi_tensor=True) and the host bookkeeping of optim.DeviceLRScale."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from helpers import ROOT

HEADER = os.path.join(ROOT, "include", "sanerf_hip.h")


def test_header_declares_and_library_exports_the_symbol():
    from sanerf_hq_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+sn_adam_step_multi\s*\(", hdr)
    assert "sn_adam_step_multi" in _lib.EXPORTED_SYMBOLS
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "sn_adam_step_multi")
    assert int(re.search(r"#define\s+SN_ADAM_MULTI_MAX_TENSORS\s+(\d+)", hdr).group(1)) == _lib.ADAM_MULTI_MAX_TENSORS >= 32
    assert int(re.search(r"#define\s+SN_ADAM_MULTI_MAX_GROUPS\s+(\d+)", hdr).group(1)) == _lib.ADAM_MULTI_MAX_GROUPS >= 8
    assert _lib.lib().sn_abi_version() == 12


def test_ctypes_records_have_the_headers_layout(tmp_path):
    """sizeof / offsetof of both records as a C compiler sees the header, against the ctypes mirror."""
    from sanerf_hq_amd import _lib
    fields = {"sn_adam_tensor": [f for f, _ in _lib.AdamTensor._fields_], "sn_adam_group": [f for f, _ in _lib.AdamGroup._fields_]}
    lines = []
    for name, fs in fields.items():
        lines.append(f'printf("{name} %zu", sizeof({name}));')
        lines += [f'printf(" %zu", offsetof({name}, {f}));' for f in fs]
        lines.append('printf("\\n");')
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sanerf_hip.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0; }\n")
    exe = tmp_path / "layout"
    subprocess.check_call([os.environ.get("CC", "cc"), "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)], text=True).splitlines()
    for line, (name, cls) in zip(out, (("sn_adam_tensor", _lib.AdamTensor), ("sn_adam_group", _lib.AdamGroup))):
        words = line.split()
        assert words[0] == name
        assert int(words[1]) == ctypes.sizeof(cls), name
        assert [int(w) for w in words[2:]] == [getattr(cls, f).offset for f in fields[name]], name


def _records(n_tensors=2, n_groups=1):
    from sanerf_hq_amd import _lib
    t = (_lib.AdamTensor * max(n_tensors, 1))()
    g = (_lib.AdamGroup * max(n_groups, 1))()
    for r in t:
        r.param, r.grad, r.exp_avg, r.exp_avg_sq, r.n, r.step_device, r.step, r.group = 16, 32, 48, 64, 8, None, 1, 0
    for r in g:
        r.lr, r.beta1, r.beta2, r.eps, r.weight_decay, r.maximize, r.flags = 1e-3, 0.9, 0.999, 1e-15, 0.0, 0, 0
    return t, g


def test_every_argument_check_answers_before_the_device_is_touched():
    from sanerf_hq_amd import _lib
    l = _lib.lib()
    call = l.sn_adam_step_multi

    def bad(t, nt, g, ng, word, scale=None, ticket=None):
        assert call(t, nt, g, ng, scale, ticket, None) == -1
        assert word in l.sn_last_error(), l.sn_last_error()

    t, g = _records()
    # nothing to do is fine: no tensors; only empty tensors (their pointers are not looked at)
    assert call(None, 0, None, 0, None, None, None) == 0
    assert call(t, 0, g, 1, None, None, None) == 0
    for r in t:
        r.n, r.param = 0, None
    assert call(t, 2, g, 1, None, None, None) == 0
    # null pointers
    t, g = _records()
    bad(None, 2, g, 1, b"host arrays")
    bad(t, 2, None, 1, b"host arrays")
    bad(t, 2, g, 0, b"group")
    for field in ("param", "grad", "exp_avg", "exp_avg_sq"):
        t, g = _records()
        setattr(t[1], field, None)
        bad(t, 2, g, 1, b"device pointers")
        setattr(t[1], field, 24)                                       # 8-byte aligned only
        bad(t, 2, g, 1, b"16-byte aligned")
    # group index, counts above the stated maximum
    t, g = _records()
    t[1].group = 1
    bad(t, 2, g, 1, b"names group 1 of 1")
    t, g = _records(_lib.ADAM_MULTI_MAX_TENSORS + 1, _lib.ADAM_MULTI_MAX_GROUPS + 1)
    bad(t, _lib.ADAM_MULTI_MAX_TENSORS + 1, g, 1, b"at most 32 per call")
    bad(t, 2, g, _lib.ADAM_MULTI_MAX_GROUPS + 1, b"at most 8 per call")
    # step counts from 1 unless the count lives on the device; one device count per tensor
    t, g = _records()
    t[0].step = 0
    bad(t, 2, g, 1, b"step counts from 1")
    t[0].step_device = 130                                             # not 4-byte aligned
    bad(t, 2, g, 1, b"4-byte aligned")
    t[0].step_device = t[1].step_device = 128
    bad(t, 2, g, 1, b"share one device step count")
    t, g = _records()
    bad(t, 2, g, 1, b"4-byte aligned", scale=18)
    bad(t, 2, g, 1, b"4-byte aligned", ticket=18)
    # hyper-parameters
    for field, value in (("beta1", 1.0), ("beta1", -0.1), ("beta2", 1.0), ("beta2", -0.1), ("lr", -1e-3), ("eps", -1e-8), ("beta1", float("nan"))):
        t, g = _records(2, 2)
        setattr(g[1], field, value)
        bad(t, 2, g, 2, b"invalid hyper-parameters (group 1)")
    t, g = _records()
    g[0].flags, g[0].weight_decay = _lib.ADAM_LAZY, 1e-3
    bad(t, 2, g, 1, b"lazy mode is defined for weight_decay = 0")


def test_constructor_rejects_what_it_rejects_today():
    from sanerf_hq_amd.optim import Adam, DeviceLRScale
    p = torch.nn.Parameter(torch.zeros(8))
    with pytest.raises(ValueError, match="amsgrad"):
        Adam([p], lr=1e-3, amsgrad=True, multi_tensor=True)
    for kw in (dict(lr=-1.0), dict(eps=-1.0), dict(betas=(1.0, 0.999)), dict(betas=(0.9, 1.0)), dict(weight_decay=-1.0)):
        with pytest.raises(ValueError, match="invalid Adam hyper-parameters"):
            Adam([p], multi_tensor=True, **kw)
    opt = Adam([p], lr=1e-3, multi_tensor=True)
    assert opt.multi_tensor and not Adam([p], lr=1e-3).multi_tensor
    assert "multi_tensor" not in opt.state_dict()["param_groups"][0], "the state_dict is the same on both routes"
    opt.step()                                                          # no gradient anywhere: nothing to do, no library call
    p.grad = torch.ones(8)
    with pytest.raises(RuntimeError, match="dense contiguous fp32 CUDA parameters only"):
        opt.step()                                                      # a CPU parameter: no silent fallback
    assert len(opt.state[p]) == 0, "a refused step leaves no state behind"
    with pytest.raises(TypeError, match="multi_tensor=True"):
        DeviceLRScale(Adam([p], lr=1e-3), lambda it: 1.0)
    with pytest.raises(TypeError):
        DeviceLRScale(torch.optim.Adam([p], lr=1e-3), lambda it: 1.0)


def test_device_lr_scale_host_bookkeeping():
    """The reference's schedule (main.py:298-303): the factor sequence, group["lr"] as LambdaLR shows it, and a state_dict round trip."""
    from sanerf_hq_amd.optim import Adam, DeviceLRScale
    iters = 4
    lam = lambda it: 0.1 ** min(it / iters, 1)                          # noqa: E731
    pa, pb = torch.nn.Parameter(torch.zeros(8)), torch.nn.Parameter(torch.zeros(3))
    qa, qb = torch.nn.Parameter(torch.zeros(8)), torch.nn.Parameter(torch.zeros(3))
    opt = Adam([dict(params=[pa], lr=1e-2), dict(params=[pb], lr=1e-3)], eps=1e-15, multi_tensor=True)
    ref = torch.optim.Adam([dict(params=[qa], lr=1e-2), dict(params=[qb], lr=1e-3)], eps=1e-15)
    sched, ref_sched = DeviceLRScale(opt, lam), torch.optim.lr_scheduler.LambdaLR(ref, lam)
    assert opt._lr_scale is not None and opt._lr_scale.dtype == torch.float32 and opt._lr_scale.numel() == 1
    with pytest.raises(RuntimeError, match="already"):
        DeviceLRScale(opt, lam)
    for it in range(7):
        assert sched.last_epoch == ref_sched.last_epoch == it
        assert sched.factor == lam(it)
        assert float(opt._lr_scale) == float(torch.tensor(lam(it), dtype=torch.float32))
        assert sched.get_last_lr() == ref_sched.get_last_lr() == [1e-2 * lam(it), 1e-3 * lam(it)]
        assert [g["lr"] for g in opt.param_groups] == [g["lr"] for g in ref.param_groups]
        assert [g["initial_lr"] for g in opt.param_groups] == [1e-2, 1e-3]
        ref.step(); ref_sched.step(); sched.step()
    assert sched.factor == 0.1 ** 1
    # round trip into a fresh optimiser + scheduler
    opt2 = Adam([dict(params=[pa], lr=1e-2), dict(params=[pb], lr=1e-3)], eps=1e-15, multi_tensor=True)
    sched2 = DeviceLRScale(opt2, lam)
    assert sched2.last_epoch == 0 and sched2.factor == 1.0
    sd = sched.state_dict()
    assert set(sd) == {"last_epoch", "base_lrs", "factor"}
    opt2.load_state_dict(opt.state_dict())
    sched2.load_state_dict(sd)
    assert sched2.last_epoch == 7 and sched2.factor == sched.factor and sched2.get_last_lr() == sched.get_last_lr()
    assert float(opt2._lr_scale) == float(opt._lr_scale)
    assert [g["initial_lr"] for g in opt2.param_groups] == [1e-2, 1e-3]
    sched2.step()
    assert sched2.last_epoch == 8 and sched2.factor == lam(8)
