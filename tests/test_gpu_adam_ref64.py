"""GPU: k_adam and k_adam_multi (csrc/optim.hip) against the fp64 statement of tests/adam_ref64.py at update precision.

ONE step from a given state, not trajectories: p, g, exp_avg, exp_avg_sq and the step count are set directly (for the optimiser class:
opt.state[p] written before step(); the capturable forms get a 0-dim device float, which the multi route packs into its own buffer
as it does for a loaded state_dict), one step runs, and the three outputs are compared with step64 element by element.  Nothing
accumulates: the only error is the kernel's own, and the bar is budget() -- derived from u = 2^-24 per rounding in adam_ref64.py, which
tests/test_adam_ref64.py shows to be attainable (the fp32 restatement uses half of it) and to reject every planted defect of MUTANTS.

  Tier A   every route -- per-tensor host counter, per-tensor capturable, multi host counter, multi capturable (ticket), multi capturable
           with a DeviceLRScale factor that is no power of two -- x every row of HYPERS (and the two CANCEL_HYPERS rows), the whole case
           table: within budget of step64, computed in float64 on the device.
  Tier B   the host-counter routes: m', v' and p' equal step32, the NumPy float32 restatement of adam_one, BIT FOR BIT on the whole table,
           underflow rows and denormals included.  (The capturable forms run pow in double on the device, which may round the two
           bias-correction scalars differently: Tier A alone holds there.)
  shapes   the smallest at which the launch logic can go wrong: per tensor n = 1 ... 5, 1023, 1024, 1027 and 2^22 + 3 * 4096 + 3 (past the
           4096-workgroup cap: the grid-stride loop, then a 3-element tail); multi: tensors of 4095, 4096, 4097, 0, 1, 3, 8191, 12289 floats
           in three groups, and one call of more than 4096 chunks.  The large tensors tile the case table; every tensor is a view into a
           longer buffer whose rest must keep its bits.
  ctypes   what the optimiser class does not reach: SN_ADAM_ZERO_GRAD on both entry points (the gradient is zero afterwards wherever it
           was not -- the cancelling elements of the table included, whose effective gradient -+g + wd p is exactly 0 -- and p, m, v are as
           without the flag), and a multi call with an n = 0 tensor between others.

Measured on an MI355X (-s prints the figures): worst error / budget p' 0.500, m' 0.500, v' 0.427 on all five routes -- the figures of step32
on the CPU, the halves being underflow rows (an error of half a denormal on a budget of one); Tier B held for p' as well as m' and v', on
both host-counter routes, all 362 rows.  The ZERO_GRAD test is what found the kernels clearing the gradient only where they had updated:
the 8 cancelling elements of the table kept their +-0.25 until both kernels were changed to clear wherever a gradient is stored.
"""
import functools

import pytest
import torch

import adam_ref64 as ref

pytestmark = pytest.mark.gpu

FACTOR = 0.1 ** 0.35                                                     # a DeviceLRScale factor that is no power of two
ROUTES = {                                                               # name -> (multi_tensor, capturable, DeviceLRScale factor)
    "per_tensor_host": (False, False, None),
    "per_tensor_capturable": (False, True, None),
    "multi_host": (True, False, None),
    "multi_capturable": (True, True, None),
    "multi_capturable_lr_scale": (True, True, FACTOR),
}
HOST_ROUTES = ("per_tensor_host", "multi_host")
# the rows the shape tests run: the reference's options at a middling count; decay + maximize early; lazy late
SHAPE_ROWS = [dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-15, weight_decay=0.0, maximize=False, lazy=False, step=7),
              dict(lr=3e-5, betas=(0.5, 0.99), eps=1e-8, weight_decay=1e-3, maximize=True, lazy=False, step=2),
              dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-15, weight_decay=0.0, maximize=True, lazy=True, step=1000)]
GUARD = 64                                                               # floats behind every tensor that no kernel may touch


@functools.lru_cache(maxsize=None)
def host_table():
    return ref.cases(0)


@functools.lru_cache(maxsize=None)
def table(gpu):
    c = host_table()
    return {k: torch.from_numpy(c[k]).to(gpu) for k in "pgmv"}


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


class Reference:
    """step64, the budget and (lazily) step32 of the case table for one row -- computed once, indexed by every tensor that tiles the table."""

    def __init__(self, gpu, h, factor=None):
        self.gpu, self.h, self.factor = gpu, h, factor
        self.r = self.b = self._bits = None

    def ratios(self, got, idx=None):
        """{key: (worst error / budget, zero-budget elements exact)} of got = dict(p, m, v); idx: the table element of each element of got."""
        if self.r is None:
            T = table(self.gpu)
            self.r = ref.step64(T["p"], T["g"], T["m"], T["v"], **self.h, lr_scale=self.factor)
            self.b = ref.budget(T["p"], T["g"], T["m"], T["v"], self.r, **self.h, lr_scale=self.factor)
        out = {}
        for k in "pmv":
            want, bound = (self.r[k], self.b[k]) if idx is None else (self.r[k][idx], self.b[k][idx])
            out[k] = ref.worst_ratio(got[k], want, bound)
        return out

    def bits(self):
        if self._bits is None:
            c = host_table()
            s = ref.step32(c["p"], c["g"], c["m"], c["v"], **self.h, lr_scale=self.factor)
            self._bits = {k: torch.from_numpy(s[k]).to(self.gpu) for k in "pmv"}
        return self._bits


@functools.lru_cache(maxsize=None)
def shape_ref(gpu, k, factor=None):
    """The reference of SHAPE_ROWS[k], shared by the shape tests."""
    return Reference(gpu, SHAPE_ROWS[k], factor)


class Item:
    """One tensor of a step: the table elements idx (all of it when None) as views into buffers with GUARD more floats behind them."""

    def __init__(self, gpu, h, idx=None):
        T = table(gpu)
        self.h, self.idx = h, idx
        src = {k: (T[k] if idx is None else T[k][idx]) for k in "pgmv"}
        self.n = src["p"].numel()
        self.buf = {k: torch.cat([a, T[k][:GUARD]]) for k, a in src.items()}
        self.before = {k: b.clone() for k, b in self.buf.items()}
        self.p, self.g, self.m, self.v = (self.buf[k][:self.n] for k in "pgmv")

    def got(self):
        return dict(p=self.p, m=self.m, v=self.v)

    def assert_rest_untouched(self, gradient_too=True):
        for k in "pgmv":
            assert same_bits(self.buf[k][self.n:], self.before[k][self.n:]), f"the kernel wrote behind the end of {k} (n = {self.n})"
        if gradient_too:
            assert same_bits(self.buf["g"], self.before["g"]), "the gradient is read only without SN_ADAM_ZERO_GRAD"


def one_step(gpu, items, route):
    """One optimiser over the items -- a parameter group per row (items that share a row object share the group) -- its state written
    directly, one step()."""
    from sanerf_hq_amd.optim import Adam, DeviceLRScale
    multi, capturable, factor = ROUTES[route]
    params = [torch.nn.Parameter(it.p) for it in items]                   # (shares the item's storage: the kernel writes through the pointer)
    groups = {}
    for q, it in zip(params, items):
        groups.setdefault(id(it.h), (it.h, []))[1].append(q)
    opt = Adam([dict(params=qs, lr=h["lr"], betas=h["betas"], eps=h["eps"], weight_decay=h["weight_decay"], maximize=h["maximize"], lazy=h["lazy"])
                for h, qs in groups.values()], capturable=capturable, multi_tensor=multi)
    if factor is not None:
        DeviceLRScale(opt, lambda it: factor)
    for q, it in zip(params, items):
        count = float(it.h["step"] - 1)
        opt.state[q] = dict(step=torch.full((), count, dtype=torch.float32, device=gpu) if capturable else torch.tensor(count),
                            exp_avg=it.m, exp_avg_sq=it.v)
        q.grad = it.g
        assert q.data_ptr() == it.p.data_ptr()
    opt.step()
    for q, it in zip(params, items):
        assert float(opt.state[q]["step"]) == it.h["step"], "the step count after the step"
        assert opt.state[q]["exp_avg"].data_ptr() == it.m.data_ptr()
    if multi and capturable:
        assert int(opt._ticket) == 0, "every launch leaves the ticket at zero"


def report(worst, ratios, where):
    for k, (ratio, exact) in ratios.items():
        assert exact, f"{k}': an element that the step must leave alone was written ({where})"
        assert ratio < 1.0, f"{k}': error / budget = {ratio:.3f} ({where})"
        worst[k] = max(worst[k], ratio)


@pytest.mark.parametrize("route", list(ROUTES))
def test_tier_a_every_route_and_row_within_budget_of_step64(gpu, route):
    rows = ref.HYPERS + ref.CANCEL_HYPERS
    factor = ROUTES[route][2]
    per_step = 8 if ROUTES[route][0] else 1                              # the multi routes: eight rows, so eight groups, in one launch
    worst = dict(p=0.0, m=0.0, v=0.0)
    for head in range(0, len(rows), per_step):
        items = [Item(gpu, h) for h in rows[head:head + per_step]]
        one_step(gpu, items, route)
        for it in items:
            report(worst, Reference(gpu, it.h, factor).ratios(it.got()), f"{route}, {ref.row_id(it.h)}")
            it.assert_rest_untouched()
    print(f"tier A {route}: worst error / budget over {len(rows)} rows x {host_table()['p'].size} elements: " + ", ".join(f"{k}' {worst[k]:.3f}" for k in "pmv"))


@pytest.mark.parametrize("route", HOST_ROUTES)
def test_tier_b_host_counter_routes_equal_step32_bit_for_bit(gpu, route):
    rows = ref.HYPERS + ref.CANCEL_HYPERS
    per_step = 8 if ROUTES[route][0] else 1
    differing = dict(p=[], m=[], v=[])
    for head in range(0, len(rows), per_step):
        items = [Item(gpu, h) for h in rows[head:head + per_step]]
        one_step(gpu, items, route)
        for it in items:
            want = Reference(gpu, it.h).bits()
            for k, got in it.got().items():
                if not same_bits(got, want[k]):
                    bad = (got.view(torch.int32) != want[k].view(torch.int32)).nonzero().squeeze(1)
                    i = int(bad[0])
                    T = table(gpu)
                    differing[k].append(f"{ref.row_id(it.h)}: {bad.numel()} elements, first {i}: p {float(T['p'][i])!r} g {float(T['g'][i])!r} "
                                        f"m {float(T['m'][i])!r} v {float(T['v'][i])!r} -> got {float(got[i])!r} want {float(want[k][i])!r}")
    for k in "pmv":
        print(f"tier B {route}: {k}' differs from step32 in {len(differing[k])} of {len(rows)} rows")
        for line in differing[k][:5]:
            print("   ", line)
    assert not differing["m"] and not differing["v"], "m' and v' are multiplies, adds and subtracts: equal under this build's flags"
    assert not differing["p"], "p' needs a correctly rounded sqrtf and division besides"


def tiled(gpu, n, offset=0):
    return (torch.arange(n, device=gpu) + offset) % host_table()["p"].size


@pytest.mark.parametrize("route", ["per_tensor_host", "per_tensor_capturable"])
def test_per_tensor_shapes(gpu, route):
    """n = 1 ... 5, 1023, 1024, 1027 (whole quads and tails, one and two workgroups) and 2^22 + 3 * 4096 + 3 floats: 4 194 304 is what the
    capped grid covers in one sweep, so the loop runs a second time for part of the grid, and a 3-element tail follows."""
    worst = dict(p=0.0, m=0.0, v=0.0)
    refs = [shape_ref(gpu, k) for k in range(3)]
    for j, n in enumerate([1, 2, 3, 4, 5, 1023, 1024, 1027, (1 << 22) + 3 * 4096 + 3]):
        for k, h in enumerate(SHAPE_ROWS):
            it = Item(gpu, h, tiled(gpu, n, offset=977 * (3 * j + k)))
            one_step(gpu, [it], route)
            report(worst, refs[k].ratios(it.got(), it.idx), f"{route}, n = {n}, {ref.row_id(h)}")
            it.assert_rest_untouched()
            if route in HOST_ROUTES:
                assert all(same_bits(got, refs[k].bits()[key][it.idx]) for key, got in it.got().items()), f"bits, n = {n}, {ref.row_id(h)}"
    print(f"shapes {route}: worst error / budget " + ", ".join(f"{k}' {worst[k]:.3f}" for k in "pmv"))


MULTI_SIZES = {"tile_edges": [4095, 4096, 4097, 0, 1, 3, 8191, 12289],    # around the 4096-float chunk; an empty tensor in the middle
               "more_chunks_than_workgroups": [4097 * 4096 + 5, 4097, 3]}  # 4098 + 2 + 1 chunks on a grid capped at 4096 workgroups


@pytest.mark.parametrize("sizes", list(MULTI_SIZES))
@pytest.mark.parametrize("route", ["multi_host", "multi_capturable", "multi_capturable_lr_scale"])
def test_multi_tensor_shapes(gpu, route, sizes, monkeypatch):
    """One call over all the tensors, in three groups with the three SHAPE_ROWS (consecutive tensors take them in turn)."""
    from sanerf_hq_amd import _lib
    factor = ROUTES[route][2]
    worst = dict(p=0.0, m=0.0, v=0.0)
    refs = [shape_ref(gpu, k, factor) for k in range(3)]
    items = [Item(gpu, SHAPE_ROWS[j % 3], tiled(gpu, n, offset=1231 * j)) for j, n in enumerate(MULTI_SIZES[sizes])]
    calls, lib = [], _lib.lib()
    real = lib.sn_adam_step_multi
    monkeypatch.setattr(lib, "sn_adam_step_multi", lambda t, nt, g, ng, *rest: (calls.append((nt, ng)), real(t, nt, g, ng, *rest))[1])
    one_step(gpu, items, route)
    assert calls == [(len(items), 3)], "one call for all the tensors, in three groups"
    for j, it in enumerate(items):
        where = f"{route}, tensor {j} of {it.n} floats, {ref.row_id(it.h)}"
        if it.n:
            report(worst, refs[j % 3].ratios(it.got(), it.idx), where)
            if route in HOST_ROUTES:
                assert all(same_bits(got, refs[j % 3].bits()[key][it.idx]) for key, got in it.got().items()), f"bits: {where}"
        it.assert_rest_untouched()
    print(f"shapes {route} {sizes}: worst error / budget " + ", ".join(f"{k}' {worst[k]:.3f}" for k in "pmv"))


# ---- through ctypes: what the optimiser class does not reach -------------------------------------------------------------------------
def zero_grad_rows():
    plain = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-15, weight_decay=1e-3, maximize=False, lazy=False, step=3)
    return ref.CANCEL_HYPERS + [plain, SHAPE_ROWS[2]]                     # the two cancelling rows, a decayed dense row, a lazy row


def zero_grad_items(gpu, h):
    """The whole table (the cancelling quads sit at its end); 3 cancelling elements (the tail path alone); 7 (a quad and a tail); one float."""
    c = host_table()["cancel"]
    first = c.start + (8 if h["maximize"] else 0)                        # the half of the block whose effective gradient is 0 under this row
    idx = [None, torch.arange(first, first + 3, device=gpu), torch.arange(first, first + 7, device=gpu), torch.arange(first, first + 1, device=gpu)]
    return [Item(gpu, h, i) for i in idx]


def call_single(it, flags):
    from sanerf_hq_amd import _lib
    h = it.h
    _lib.check(_lib.lib().sn_adam_step(it.p.data_ptr(), it.g.data_ptr(), it.m.data_ptr(), it.v.data_ptr(), it.n, h["lr"], h["betas"][0], h["betas"][1],
                                       h["eps"], h["weight_decay"], h["step"], None, int(h["maximize"]),
                                       flags | (_lib.ADAM_LAZY if h["lazy"] else 0), _lib.stream()), "sn_adam_step")


def call_multi(items, flags, gpu, with_empty=True):
    """One sn_adam_step_multi over the items, a group each; with_empty: an n = 0 tensor with null pointers after the first."""
    from sanerf_hq_amd import _lib
    order = list(items[:1]) + ([None] if with_empty else []) + list(items[1:])
    trec, grec = (_lib.AdamTensor * len(order))(), (_lib.AdamGroup * len(items))()
    gi = 0
    for r, it in zip(trec, order):
        if it is None:
            r.param = r.grad = r.exp_avg = r.exp_avg_sq = r.step_device = None
            r.n, r.step, r.group = 0, 1, 0
            continue
        h, g = it.h, grec[gi]
        g.lr, g.beta1, g.beta2, g.eps, g.weight_decay = h["lr"], h["betas"][0], h["betas"][1], h["eps"], h["weight_decay"]
        g.maximize, g.flags = int(h["maximize"]), flags | (_lib.ADAM_LAZY if h["lazy"] else 0)
        r.param, r.grad, r.exp_avg, r.exp_avg_sq, r.n = it.p.data_ptr(), it.g.data_ptr(), it.m.data_ptr(), it.v.data_ptr(), it.n
        r.step_device, r.step, r.group = None, h["step"], gi
        gi += 1
    _lib.check(_lib.lib().sn_adam_step_multi(trec, len(order), grec, len(items), None, None, _lib.stream()), "sn_adam_step_multi")


@pytest.mark.parametrize("entry", ["sn_adam_step", "sn_adam_step_multi"])
def test_zero_grad_flag_clears_every_gradient_and_changes_nothing_else(gpu, entry):
    """SN_ADAM_ZERO_GRAD: "the gradient is cleared in the same pass".  After the call every gradient element is zero -- also where the
    kernel has nothing to update: a quad (or tail element) whose effective gradient -+g + wd p cancels to exactly 0 on zero moments still
    holds a non-zero raw gradient, and an accumulating caller would add the next step's on top of it.  p, m and v are, bit for bit, what
    the call without the flag gives, which in turn is within budget of step64; without the flag the gradient is not written."""
    from sanerf_hq_amd import _lib
    worst = dict(p=0.0, m=0.0, v=0.0)
    for h in zero_grad_rows():
        plain, flagged = zero_grad_items(gpu, h), zero_grad_items(gpu, h)
        if entry == "sn_adam_step":
            for it in plain:
                call_single(it, 0)
            for it in flagged:
                call_single(it, _lib.ADAM_ZERO_GRAD)
        else:
            call_multi(plain, 0, gpu)
            call_multi(flagged, _lib.ADAM_ZERO_GRAD, gpu)
        R = Reference(gpu, h)
        for a, b in zip(plain, flagged):
            where = f"{entry}, n = {a.n}, {ref.row_id(h)}"
            report(worst, R.ratios(a.got(), a.idx), where)
            a.assert_rest_untouched()
            assert all(same_bits(x, y) for x, y in zip(a.got().values(), b.got().values())), f"the flag changed the update ({where})"
            b.assert_rest_untouched(gradient_too=False)
            left = int((b.g != 0).sum())
            assert left == 0, f"{left} of {b.n} gradient elements survive SN_ADAM_ZERO_GRAD ({where}; {int((a.g != 0).sum())} were non-zero)"
    print(f"{entry}: worst error / budget " + ", ".join(f"{k}' {worst[k]:.3f}" for k in "pmv"))


def test_multi_call_with_an_empty_tensor_between_two_others(gpu):
    """sanerf_hip.h: "n = 0 is fine" -- null pointers and all, between tensors of other groups: the others get the update of the
    per-tensor entry point bit for bit, and of step64 within budget."""
    worst = dict(p=0.0, m=0.0, v=0.0)
    sizes = [4097, 5]
    multi = [Item(gpu, h, tiled(gpu, n, offset=311)) for h, n in zip(SHAPE_ROWS, sizes)]
    single = [Item(gpu, h, tiled(gpu, n, offset=311)) for h, n in zip(SHAPE_ROWS, sizes)]
    call_multi(multi, 0, gpu, with_empty=True)
    for it in single:
        call_single(it, 0)
    for a, b in zip(multi, single):
        report(worst, Reference(gpu, a.h).ratios(a.got(), a.idx), f"n = {a.n}, {ref.row_id(a.h)}")
        assert all(same_bits(x, y) for x, y in zip(a.got().values(), b.got().values()))
        a.assert_rest_untouched()
    # ... and a call of nothing but empty tensors launches nothing and is fine
    from sanerf_hq_amd import _lib
    trec, grec = (_lib.AdamTensor * 2)(), (_lib.AdamGroup * 1)()
    for r in trec:
        r.n, r.step, r.group = 0, 1, 0
    grec[0].lr, grec[0].beta1, grec[0].beta2, grec[0].eps = 1e-3, 0.9, 0.999, 1e-15
    _lib.check(_lib.lib().sn_adam_step_multi(trec, 2, grec, 1, None, None, _lib.stream()), "sn_adam_step_multi")
    torch.cuda.synchronize()
    print("empty tensor between two others: worst error / budget " + ", ".join(f"{k}' {worst[k]:.3f}" for k in "pmv"))
