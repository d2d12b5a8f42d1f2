"""An fp64 statement of the multiresolution grid encoder for the tests, and the fp32 round-off bounds that go with it.

Written for the tests alone: nothing here imports oracle/ or the package's encoders.  It states the algorithm of
tools/gen_kat_encoders.py (gridencoder.cu:45-79 index, :94-201 forward, :205-248 dy_dx, :264-348 table gradient,
:352-378 input gradient) as vectorised torch that runs on any device, so that 4 M samples are a few index_add_ calls:

  * index arithmetic in int64, masked to 32 bits where the CUDA source computes in uint32 (coordinates < 2^24 and
    primes < 2^32: the products fit an int64);
  * kept in fp32, because they decide WHICH rows a sample touches and every implementation necessarily has them in
    fp32: the per-level resolution ceil(exp2f(l * S) * H), the position fma(x, res, -0.5) (x * (res - 1) with
    align_corners), its clamp, the cell and the fraction pos - cell (exact in fp32);
  * everything after that -- smoothstep, corner weights, blends, sums -- in float64.

Next to every result it returns what a derived error bound needs, all from the fp64 side: per table row the number of
contributions n and the absolute mass M = sum |w * g|, per output element sum |w * v|.

Bounds (u = 2^-24, first-order count of the fp32 roundings, factor 2 of margin):
  table gradient  2 (n + 2 D + s) u M       n additions in any order; 2 D: the D roundings of `1 - pos` and the D - 1
                                            products of a corner weight, and the product w * g
  forward         2 (2^D + 2 D + s) u sum|w v|
  dy_dx           2 (2^(D-1) + 2 D + 2 + s) u sum|w (v_r - v_l) deriv|
  input gradient  the dy_dx count + L C further terms, on sum |g| * (dy_dx mass)
s = 0 for linear interpolation.  Smoothstep: s = 3 D, and the masses use widened weights -- see _factors().

The two regularisers that act on the table's gradient in place are stated here too: tv_gradient() (gridencoder.cu:525-631) with
tv_bound(), weight_decay() (gridencoder.cu:670-703) with weight_decay_bound(); their counts are derived in those docstrings.
"""
import math

import torch

PRIMES = (1, 2654435761, 805459861, 3674653429, 2097192037)      # gridencoder.cu:49
M32 = 0xFFFFFFFF
U = 2.0 ** -24


class Grid:
    """Level table of one encoder: offsets as GridEncoder.__init__ lays them out (grid.py:103-142, float64 resolution for the
    allocation), kernel-side resolutions as gridencoder.cu:132-133 computes them (fp32)."""

    def __init__(self, D, L, C, log2T, base, desired=None, per_level_scale=2.0, gridtype=0, align_corners=False, interp=0):
        assert 2 <= D <= 5 and L >= 1
        scale = float(per_level_scale) if desired is None else 2.0 ** (math.log2(desired / base) / (L - 1))
        self.D, self.L, self.C, self.base, self.scale = D, L, C, int(base), scale
        self.gridtype, self.align_corners, self.interp = int(gridtype), bool(align_corners), int(interp)
        offs = [0]
        for l in range(L):
            r = int(math.ceil(base * scale ** l))
            offs.append(offs[-1] + int(math.ceil(min(2 ** log2T, r ** D) / 8) * 8))
        self.offsets = offs
        self.S = float(torch.tensor(math.log2(scale), dtype=torch.float32))            # what the ABI takes: (float)log2(per_level_scale)
        self.res = [self._kernel_res(l) for l in range(L)]
        # the dense walk of gridencoder.cu:66-70 (uint32 stride) does not depend on the sample: dims it takes, and whether the level hashes
        self.walk, self.hashed = [], []
        for l in range(L):
            size, stride, nd = self.size(l), 1, 0
            while nd < D and stride <= size:
                stride = (stride * self.res[l]) & M32
                nd += 1
            self.walk.append(nd)
            self.hashed.append(self.gridtype == 0 and stride > size)

    def size(self, l):
        return self.offsets[l + 1] - self.offsets[l]

    @property
    def rows(self):
        return self.offsets[-1]

    def _kernel_res(self, l):
        S = torch.tensor(self.S, dtype=torch.float32)
        arg = torch.tensor(float(l), dtype=torch.float32) * S                            # fp32 product
        # exp2 in float64 rounded once = a correctly rounded exp2f, like kernel_res of tools/gen_kat_encoders.py.  Where the product lands
        # within an ulp above an integer (desired = 24 from base 4 over 3 levels: 24.0000018) the ceil depends on that last bit; the tests
        # compare these resolutions with the oracle's host computation, and a kernel built on another resolution misses every bound.
        e64 = torch.exp2(arg.double())
        v = e64.float() * torch.tensor(float(self.base), dtype=torch.float32)           # exp2 rounded once, fp32 product
        return int(torch.ceil(v))


def in_range(x):
    """gridencoder.cu:105-130: a sample with any coordinate outside [0, 1] gives zeros and receives / sends no gradient."""
    return ~((x < 0) | (x > 1)).any(dim=1)


def _locate(grid, x, l):
    """cell [B, D] int64 and the fp32 fraction as float64 [B, D] (gridencoder.cu:137-149)."""
    res = grid.res[l]
    if grid.align_corners:
        pos = x * torch.tensor(float(res - 1), dtype=torch.float32, device=x.device)    # one fp32 rounding
        cell = torch.clamp(torch.floor(pos), max=float(res - 2))
    else:
        # x * res - 0.5 is exact in float64 wherever it is not clamped to 0 anyway (24 x 24 significant bits): one rounding, like the fma
        pos = (x.double() * float(res) - 0.5).float()
        pos = torch.clamp(pos, min=0.0, max=float(res - 1))
        cell = torch.floor(pos)
    frac = (pos - cell).double()                                                         # exact in fp32
    return cell.long(), frac


def _factors(grid, frac):
    """Per dimension: the interpolation factor of the lower / upper corner (lo, hi), the factors that the MASSES use (lo_m, hi_m) and
    the derivative of hi.  Linear: hi = frac is exact in fp32 and lo = 1 - frac has one rounding, a relative error: masses use the
    factors themselves.  Smoothstep: hi = f f (3 - 2 f) carries 3 relative roundings, but lo = 1 - hi inherits hi's ABSOLUTE error,
    3 u hi + u lo, which is not small relative to lo when lo is: that is <= 4 u max(lo, hi), so the masses take max(lo, hi) for the
    lower corner and the count grows by 3 per dimension (3 D in all)."""
    if grid.interp == 1:
        hi = frac * frac * (3.0 - 2.0 * frac)
        lo = 1.0 - hi
        return lo, hi, torch.maximum(lo, hi), hi, 6.0 * frac * (1.0 - frac)
    lo = 1.0 - frac
    return lo, frac, lo, frac, torch.ones_like(frac)


def _extra(grid):
    return 3 * grid.D if grid.interp == 1 else 0


def _rows(grid, l, p):
    """Table row (absolute, level offset included) of the vertices p: list of D int64 [B] (gridencoder.cu:55-79)."""
    res, size = grid.res[l], grid.size(l)
    if grid.hashed[l]:
        idx = torch.zeros_like(p[0])
        for d in range(grid.D):
            idx = idx ^ ((p[d] * PRIMES[d]) & M32)
    else:
        idx, stride = torch.zeros_like(p[0]), 1
        for d in range(grid.walk[l]):
            idx = (idx + p[d] * stride) & M32
            stride = (stride * res) & M32
    return grid.offsets[l] + idx % size


def _corner(grid, l, cell, lo, hi, lo_m, hi_m, corner, dims):
    """Weight, mass weight and vertex coordinates (only for `dims`) of one corner."""
    res = grid.res[l]
    w = torch.ones_like(lo[:, 0])
    wm = torch.ones_like(w)
    p = {}
    for k, d in enumerate(dims):
        if (corner >> k) & 1:
            w = w * hi[:, d]; wm = wm * hi_m[:, d]
            p[d] = torch.clamp(cell[:, d] + 1, max=res - 1)                              # gridencoder.cu:182
        else:
            w = w * lo[:, d]; wm = wm * lo_m[:, d]
            p[d] = cell[:, d]
    return w, wm, p


def forward(grid, x, table, want_dy_dx=False, max_level=None):
    """x [B, D] fp32, table [rows, C] fp32 or fp16 (read exactly) -> dict of float64 tensors:
    y, y_mass [B, L, C];  with want_dy_dx also dy_dx, dy_dx_mass [B, L, D, C].  Levels >= max_level and out-of-range samples are zero."""
    B, D, L, C = x.shape[0], grid.D, grid.L, grid.C
    max_level = L if max_level is None else min(max_level, L)
    ok = in_range(x)
    xs = torch.where(ok[:, None], x, torch.full_like(x, 0.5))
    okd = ok.double()[:, None]
    T = table.double()
    y = torch.zeros(B, L, C, dtype=torch.float64, device=x.device)
    ym = torch.zeros_like(y)
    dd = torch.zeros(B, L, D, C, dtype=torch.float64, device=x.device) if want_dy_dx else None
    ddm = torch.zeros_like(dd) if want_dy_dx else None
    for l in range(max_level):
        cell, frac = _locate(grid, xs, l)
        lo, hi, lo_m, hi_m, deriv = _factors(grid, frac)
        for corner in range(1 << D):
            w, wm, p = _corner(grid, l, cell, lo, hi, lo_m, hi_m, corner, list(range(D)))
            v = T[_rows(grid, l, [p[d] for d in range(D)])]
            y[:, l] += okd * w[:, None] * v
            ym[:, l] += okd * wm[:, None] * v.abs()
        if want_dy_dx:
            scale = float(grid.res[l] - 1 if grid.align_corners else grid.res[l])        # gridencoder.cu:215
            for gd in range(D):
                others = [d for d in range(D) if d != gd]
                for corner in range(1 << (D - 1)):
                    w, wm, p = _corner(grid, l, cell, lo, hi, lo_m, hi_m, corner, others)
                    p[gd] = cell[:, gd]
                    left = T[_rows(grid, l, [p[d] for d in range(D)])]
                    p[gd] = torch.clamp(cell[:, gd] + 1, max=grid.res[l] - 1)
                    diff = T[_rows(grid, l, [p[d] for d in range(D)])] - left
                    dd[:, l, gd] += okd * (scale * w * deriv[:, gd])[:, None] * diff
                    ddm[:, l, gd] += okd * (scale * wm * deriv[:, gd])[:, None] * diff.abs()
    out = dict(y=y, y_mass=ym)
    if want_dy_dx:
        out.update(dy_dx=dd, dy_dx_mass=ddm)
    return out


def backward_table(grid, x, grad, max_level=None):
    """x [B, D] fp32, grad indexable as [B, L, C] (any strides, fp32 or fp64) -> dict: grad_table [rows, C] float64, n [rows] int64 contributions
    per row (zero-weight corners count: they are added too), mass [rows, C] = sum |w * g| with the mass weights."""
    D, L, C = grid.D, grid.L, grid.C
    max_level = L if max_level is None else min(max_level, L)
    ok = in_range(x)
    sel = ok.nonzero().squeeze(1)
    xs = x[sel]
    gt = torch.zeros(grid.rows, C, dtype=torch.float64, device=x.device)
    mass = torch.zeros_like(gt)
    n = torch.zeros(grid.rows, dtype=torch.int64, device=x.device)
    for l in range(max_level):
        cell, frac = _locate(grid, xs, l)
        lo, hi, lo_m, hi_m, _ = _factors(grid, frac)
        g = grad[:, l][sel].double()
        ga = g.abs()
        for corner in range(1 << D):
            w, wm, p = _corner(grid, l, cell, lo, hi, lo_m, hi_m, corner, list(range(D)))
            rows = _rows(grid, l, [p[d] for d in range(D)])
            gt.index_add_(0, rows, w[:, None] * g)
            mass.index_add_(0, rows, wm[:, None] * ga)
            n += torch.bincount(rows, minlength=grid.rows)
    return dict(grad_table=gt, n=n, mass=mass)


def sample_rows(grid, x, max_level=None):
    """Yields, per level < max_level and corner, the table rows [B] that the samples x (all in range) touch."""
    D = grid.D
    for l in range(grid.L if max_level is None else min(max_level, grid.L)):
        cell, frac = _locate(grid, x, l)
        lo, hi, lo_m, hi_m, _ = _factors(grid, frac)
        for corner in range(1 << D):
            _, _, p = _corner(grid, l, cell, lo, hi, lo_m, hi_m, corner, list(range(D)))
            yield _rows(grid, l, [p[d] for d in range(D)])


def contributions(grid, x, max_level=None):
    """n [rows] int64 alone: contributions per table row of the in-range samples of x."""
    n = torch.zeros(grid.rows, dtype=torch.int64, device=x.device)
    for rows in sample_rows(grid, x[in_range(x)], max_level):
        n += torch.bincount(rows, minlength=grid.rows)
    return n


def min_over_rows(grid, x, row_values, max_level=None):
    """[B] float64: per sample the smallest of row_values [rows] over the rows its corners touch (+inf for out-of-range samples)."""
    ok = in_range(x)
    m = torch.full((int(ok.sum()),), float("inf"), dtype=torch.float64, device=x.device)
    for rows in sample_rows(grid, x[ok], max_level):
        m = torch.minimum(m, row_values[rows])
    out = torch.full((x.shape[0],), float("inf"), dtype=torch.float64, device=x.device)
    out[ok] = m
    return out


def backward_input(grid, grad, fwd):
    """grad indexable as [B, L, C], fwd = forward(..., want_dy_dx=True) -> dict: grad_inputs [B, D] float64, mass [B, D]
    (gridencoder.cu:352-378: sum over levels and channels of grad * dy_dx)."""
    g = grad.double()[:, :, None, :]
    return dict(grad_inputs=(g * fwd["dy_dx"]).sum(dim=(1, 3)), mass=(g.abs() * fwd["dy_dx_mass"]).sum(dim=(1, 3)))


# ---- the regularisers on the table gradient ---------------------------------------------------------------------------------------
TV_EPS = float(torch.tensor(1e-9, dtype=torch.float32))                                  # the literal 1e-9f of gridencoder.cu:628, widened


def tv_cells(grid, x, l):
    """Centre vertex [B, D] int64 of the samples x (all in range) on level l: gridencoder.cu:566-576, the same fp32 position and floor
    as the encoder's (_locate) -- min(floor, res - 2) with align_corners, else the floor of the clamped position, which reaches res - 1."""
    return _locate(grid, x, l)[0]


def tv_gradient(grid, x, table, weight):
    """What kernel_grad_tv ADDS to the table gradient (gridencoder.cu:525-631), in float64.  x [B, D] fp32 in [0, 1] (samples outside
    contribute nothing, :547-557), table [rows, C] read exactly, weight a Python float -> dict:
      grad [rows, C] float64   sum over samples and levels of  w * results / sqrt(idelta + eps)  at the row of the sample's centre vertex,
                               results = sum of (centre - neighbour) over the neighbours, idelta = sum of their squares (:588-629)
      n    [rows]    int64     contributions per row
      mass [rows, C] float64   M = sum |w| * (sum over the neighbours of |centre - neighbour|) / sqrt(idelta + eps)
    Neighbours: per dimension the vertex at +1 ALWAYS -- the guard `cur_d < resolution` (:595) cannot fail, so a centre at res - 1 asks
    for the vertex res, one past the last, which get_grid_index folds back by its unconditional `% hashmap_size` (:78; _rows does the
    same) -- and the vertex at -1 where the centre is not 0 (:608).
    w = weight / (2 D) is rounded to fp32 (:586: a float), eps is the fp32 literal 1e-9f.

    Departures of the HIP kernel from the reference's text that this statement is indifferent to, and that are deliberate: it spells the
    accumulation idelta += gv * gv as an fmaf (nvcc contracts the reference's line to one), 1 / sqrtf for rsqrtf (IEEE-rounded both, where
    rsqrtf is an approximation), and it forces the generic modulo on every level, because the level's own addressing mode (none on a dense
    level, a mask on a power of two) does not cover the vertex res."""
    D, C = grid.D, grid.C
    dev = x.device
    xs = x[in_range(x)]
    T = table.double()
    w = float(torch.tensor(weight, dtype=torch.float32) / torch.tensor(float(2 * D), dtype=torch.float32))
    gt = torch.zeros(grid.rows, C, dtype=torch.float64, device=dev)
    mass = torch.zeros_like(gt)
    n = torch.zeros(grid.rows, dtype=torch.int64, device=dev)
    for l in range(grid.L):
        cell = tv_cells(grid, xs, l)
        p = [cell[:, d] for d in range(D)]
        centre = _rows(grid, l, p)
        c = T[centre]
        results, idelta, absum = torch.zeros_like(c), torch.zeros_like(c), torch.zeros_like(c)
        for d in range(D):
            q = list(p)
            q[d] = p[d] + 1                                                              # up to and including the vertex `res`
            gv = c - T[_rows(grid, l, q)]
            results += gv; idelta += gv * gv; absum += gv.abs()
            has_left = (p[d] > 0).double()[:, None]
            q[d] = torch.clamp(p[d] - 1, min=0)
            gv = (c - T[_rows(grid, l, q)]) * has_left
            results += gv; idelta += gv * gv; absum += gv.abs()
        inv = 1.0 / torch.sqrt(idelta + TV_EPS)
        gt.index_add_(0, centre, w * results * inv)
        mass.index_add_(0, centre, abs(w) * absum * inv)
        n += torch.bincount(centre, minlength=grid.rows)
    return dict(grad=gt, n=n, mass=mass)


def level_of_rows(grid, device=None):
    """[rows] int64: the level whose [offsets[l], offsets[l+1]) holds the row -- what the binary search of gridencoder.cu:686-699 finds."""
    sizes = torch.tensor([grid.size(l) for l in range(grid.L)], dtype=torch.int64, device=device)
    return torch.repeat_interleave(torch.arange(grid.L, dtype=torch.int64, device=device), sizes)


def weight_decay(grid, table, weight):
    """What kernel_grad_wd ADDS (gridencoder.cu:670-703): 2 * weight * table / size(level of the row), float64 [rows, C]; weight is
    rounded to fp32 (the kernel's argument is a float)."""
    w = float(torch.tensor(weight, dtype=torch.float32))
    sizes = torch.tensor([float(grid.size(l)) for l in range(grid.L)], dtype=torch.float64, device=table.device)
    return 2.0 * w * table.double() / sizes[level_of_rows(grid, table.device)][:, None]


def weight_decay_exact_levels(grid, device=None):
    """[rows, C] fp32: 1.0f / size(level of the row) -- what a table of ones, a zero gradient and weight 0.5 must give to the bit
    (2 * 0.5 * 1 = 1 exactly, one correctly rounded division, 0 + v = v)."""
    sizes = torch.tensor([float(grid.size(l)) for l in range(grid.L)], dtype=torch.float32, device=device)
    one = torch.ones((), dtype=torch.float32, device=device)
    return (one / sizes)[level_of_rows(grid, device)][:, None].expand(grid.rows, grid.C).contiguous()


# ---- bounds: every count in one place ---------------------------------------------------------------------------------------------
def forward_bound(grid, y_mass):
    return 2.0 * ((1 << grid.D) + 2 * grid.D + _extra(grid)) * U * y_mass


def dy_dx_terms(grid):
    """2^(D-1) accumulations, 2 D for the weight as in the forward, 2 for v_r - v_l and the product with the derivative."""
    return (1 << (grid.D - 1)) + 2 * grid.D + 2 + _extra(grid)


def dy_dx_bound(grid, dy_dx_mass):
    return 2.0 * dy_dx_terms(grid) * U * dy_dx_mass


def input_grad_bound(grid, mass):
    return 2.0 * (dy_dx_terms(grid) + grid.L * grid.C) * U * mass


def table_grad_bound(grid, n, mass):
    """[rows, C]; rows with n = 0 get a bound of exactly 0."""
    return 2.0 * (n.double() + 2 * grid.D + _extra(grid))[:, None] * U * mass


def tv_terms(grid):
    """fp32 roundings behind ONE contribution t = w * r * q, r = results, q = 1 / sqrt(idelta + eps), counted in units of
    u * m with m = |w| * A * q and A = sum over the k <= 2 D neighbours of |gv| (so |t| <= m), to first order:
      1      every difference gv = centre - neighbour is rounded once: each |gv| is off by <= u |gv|, r by <= u A;
      2 D    the (at most 2 D) additions into `results`: each rounds a partial sum that is <= A in magnitude.  This is an ABSOLUTE
             error <= 2 D u A on r, however small |r| is after cancellation -- which is why the mass is built on A, not on |r|;
      D + 1  idelta: a sum of non-negative terms, so relative errors add: 2 u from the two roundings inside gv * gv (the rounded
             difference enters squared), and one rounding per fused multiply-add, 2 D of them: (2 D + 2) u on idelta; the square root
             halves it;
      1/2    the addition of eps rounds once, halved by the root as well;
      2      sqrtf: 1 ulp, which is up to 2 u relative, in the HIP math API's table of single-precision functions (the product library
             builds it correctly rounded, 1/2 ulp; the documented figure is what is counted);
      1      the division 1 / sqrt: correctly rounded;
      2      the two products w * r and (w * r) * q.
    Sum: 3 D + 7.5, taken as 3 D + 8.  (rsqrtf, the reference's own spelling, is 1 ulp in the same table and saves the division:
    a kernel written that way fits the same count.)"""
    return 3 * grid.D + 8


def tv_bound(grid, n, mass, g0=None):
    """[rows, C] bound on |(got - g0) - tv_gradient()["grad"]|:  2 u ((n + 3 D + 8) M + n |g0|).
    The n contributions of a row are added to the gradient that is already there, g0, by atomics in any order: n additions, each rounding a
    partial sum that is at most |g0| + M in magnitude, which is n u (|g0| + M); without g0 the gradient is taken to start at zero.
    The contributions themselves carry tv_terms() roundings each, relative to their masses, which sum to M.  Factor 2 of margin as
    everywhere in this module.  Rows with n = 0 get a bound of exactly 0: they must keep g0 bit for bit."""
    nd = n.double()[:, None]
    b = (nd + tv_terms(grid)) * mass
    if g0 is not None:
        b = b + nd * g0.double().abs()
    return 2.0 * U * b


def weight_decay_bound(grid, g0, term):
    """|got - (g0 + term)| <= 2 * 4 u (|g0| + |term|): 2 * weight is exact; the product with the table value, the division by the size and the
    final addition round once each (the first two relative to |term|, the last to |g0 + term|), and the conversion of a size above 2^24 to
    fp32 would be a fourth."""
    return 2.0 * 4 * U * (g0.double().abs() + term.abs())


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound over the elements with a positive bound, and whether every element with bound 0 is met exactly."""
    err = (got.double() - ref).abs()
    pos = bound > 0
    ratio = float((err[pos] / bound[pos]).max()) if bool(pos.any()) else 0.0
    exact = bool((err[~pos] == 0).all())
    return ratio, exact
