"""CPU: sn_ema_update_multi (the parameter average of every tracked tensor in one launch) and optim.ParamEMA as far as they go without a
GPU -- the symbol, the layout of its record, every host-side argument check (all of them run before anything touches the device), what
the class refuses, and the 'ema' entry of a checkpoint."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from helpers import ROOT, make_opt

HEADER = os.path.join(ROOT, "include", "sanerf_hip.h")


def test_header_declares_and_library_exports_the_symbol():
    from sanerf_hq_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+sn_ema_update_multi\s*\(", hdr)
    assert "sn_ema_update_multi" in _lib.EXPORTED_SYMBOLS
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "sn_ema_update_multi")
    assert int(re.search(r"#define\s+SN_EMA_MULTI_MAX_TENSORS\s+(\d+)", hdr).group(1)) == _lib.EMA_MULTI_MAX_TENSORS == 32
    assert int(re.search(r"#define\s+SN_EMA_ADVANCE\s+(\d+)", hdr).group(1)) == _lib.EMA_ADVANCE == 1


def test_the_abi_version_is_still_12():
    """The entry point is an addition: nothing that existed moved."""
    from sanerf_hq_amd import _lib
    hdr = open(HEADER).read()
    assert int(re.search(r"#define\s+SN_ABI_VERSION\s+(\d+)", hdr).group(1)) == 12
    assert _lib.ABI_VERSION == 12 and _lib.lib().sn_abi_version() == 12


def test_ctypes_record_has_the_headers_layout(tmp_path):
    """sizeof / offsetof of the record as a C compiler sees the header, against the ctypes mirror."""
    from sanerf_hq_amd import _lib
    fields = [f for f, _ in _lib.EmaTensor._fields_]
    assert fields == ["shadow", "param", "n"]
    lines = ['printf("%zu", sizeof(sn_ema_tensor));'] + [f'printf(" %zu", offsetof(sn_ema_tensor, {f}));' for f in fields] + ['printf("\\n");']
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sanerf_hip.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0; }\n")
    exe = tmp_path / "layout"
    subprocess.check_call([os.environ.get("CC", "cc"), "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)])
    words = [int(w) for w in subprocess.check_output([str(exe)], text=True).split()]
    assert words[0] == ctypes.sizeof(_lib.EmaTensor) == 24
    assert words[1:] == [getattr(_lib.EmaTensor, f).offset for f in fields]


def _records(n=2):
    from sanerf_hq_amd import _lib
    t = (_lib.EmaTensor * max(n, 1))()
    for i, r in enumerate(t):
        r.shadow, r.param, r.n = 4096 + 64 * i, 8192 + 64 * i, 8
    return t


def test_every_argument_check_answers_before_the_device_is_touched():
    """The pointers below are no device addresses: a call that got as far as a launch would not answer -1 with these texts."""
    from sanerf_hq_amd import _lib
    l = _lib.lib()
    call = l.sn_ema_update_multi
    ADV = _lib.EMA_ADVANCE

    def bad(word, t, nt, decay=0.95, count=None, ticket=None, flags=0):
        assert call(t, nt, decay, count, ticket, flags, None) == -1
        assert word in l.sn_last_error(), l.sn_last_error()

    t = _records()
    # nothing to do is fine: no tensors; only empty tensors (their pointers are not looked at); no count to advance
    assert call(None, 0, 0.95, None, None, 0, None) == 0
    assert call(t, 0, 0.95, None, None, 0, None) == 0
    for r in t:
        r.n, r.shadow, r.param = 0, None, None
    assert call(t, 2, 0.95, None, None, 0, None) == 0
    assert call(t, 2, 0.95, 64, 32, 0, None) == 0                       # a count and a ticket, nothing to update, nothing to advance: no launch
    # more tensors than one call takes
    t = _records(_lib.EMA_MULTI_MAX_TENSORS + 1)
    bad(b"at most 32 per call", t, _lib.EMA_MULTI_MAX_TENSORS + 1)
    # pointers
    bad(b"host array", None, 2)
    for field in ("shadow", "param"):
        t = _records()
        setattr(t[1], field, None)
        bad(b"device pointers (tensor 1)", t, 2)
        setattr(t[1], field, 4096 + 24)                                 # 8-byte aligned only
        bad(b"16-byte aligned (tensor 1)", t, 2)
    t = _records()
    t[1].param = t[1].shadow
    bad(b"same tensor (tensor 1)", t, 2)
    # decay
    t = _records()
    for decay in (-0.01, 1.01, float("nan"), float("inf")):
        bad(b"decay must lie in [0, 1]", t, 2, decay=decay)
    # the count, the ticket and the flag
    bad(b"needs a ticket", t, 2, count=64, flags=ADV)
    bad(b"needs num_updates_device", t, 2, ticket=32, flags=ADV)
    bad(b"needs num_updates_device", t, 0, ticket=32, flags=ADV)
    bad(b"8-byte aligned", t, 2, count=68, ticket=32, flags=ADV)
    bad(b"8-byte aligned", t, 2, count=68)
    bad(b"4-byte aligned", t, 2, count=64, ticket=34, flags=ADV)
    bad(b"4-byte aligned", t, 2, ticket=34)
    bad(b"unknown flags", t, 2, flags=2)


def test_the_class_rejects_what_it_cannot_average():
    """CPU, non-fp32 and non-contiguous tensors, in the constructor and handed to update(); a decay outside [0, 1]."""
    from sanerf_hq_amd.optim import ParamEMA
    ok = torch.nn.Parameter(torch.zeros(8))
    for decay in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="between 0 and 1"):
            ParamEMA([ok], decay)
    cpu = torch.nn.Parameter(torch.zeros(8))
    half = torch.nn.Parameter(torch.zeros(8, dtype=torch.float16))
    strided = torch.nn.Parameter(torch.zeros(8, 8).t()[:, :4])
    for p in (cpu, half, strided):
        with pytest.raises(RuntimeError, match="dense contiguous fp32 CUDA parameters only"):
            ParamEMA([p], 0.95)
    # update() with tensors of its own: the same refusals, before anything is written (an instance without going through the device)
    ema = ParamEMA.__new__(ParamEMA)
    ema.decay, ema.on_write, ema._params, ema.collected_params, ema._use_count, ema._recs = 0.95, None, [], None, False, None
    ema.shadow_params = [torch.full((8,), 3.0)]
    for p in (cpu, half, strided):
        with pytest.raises(RuntimeError, match="dense contiguous fp32 CUDA parameters only"):
            ema.update([p])
        with pytest.raises(RuntimeError, match="dense contiguous fp32 CUDA parameters only"):
            ema.copy_to([p])
    with pytest.raises(ValueError, match="different from number of shadow parameters"):
        ema.update([cpu, cpu])
    with pytest.raises(RuntimeError, match="no `store\\(\\)`ed weights"):
        ema.restore([cpu])
    assert torch.equal(ema.shadow_params[0], torch.full((8,), 3.0)) and not cpu.any()


class _FakeEMA:
    def state_dict(self):
        return {"decay": 0.95, "num_updates": 7, "shadow_params": [torch.ones(3)], "collected_params": None}


def test_save_checkpoint_adds_exactly_the_ema_entry(tmp_path):
    from sanerf_hq_amd.nerf import NeRFNetwork
    from sanerf_hq_amd.nerf.utils import save_checkpoint
    model = NeRFNetwork(make_opt())
    plain = save_checkpoint(model, str(tmp_path / "a.pth"), epoch=1, global_step=2)
    assert set(plain) == {"epoch", "global_step", "stats", "model"}
    assert set(torch.load(str(tmp_path / "a.pth"), weights_only=False)) == set(plain)
    with_ema = save_checkpoint(model, str(tmp_path / "b.pth"), epoch=1, global_step=2, ema=_FakeEMA())
    assert set(with_ema) == set(plain) | {"ema"}
    loaded = torch.load(str(tmp_path / "b.pth"), weights_only=False)
    assert set(loaded) == set(plain) | {"ema"}
    assert list(loaded["ema"]) == ["decay", "num_updates", "shadow_params", "collected_params"]
    assert loaded["ema"]["decay"] == 0.95 and loaded["ema"]["num_updates"] == 7 and torch.equal(loaded["ema"]["shadow_params"][0], torch.ones(3))
