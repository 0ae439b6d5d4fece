"""-m gpu: the fused clip + Adam launches (csrc/estimator_ops.hip: adam_kernel, adam8_kernel) in the full form the engine's update uses --
gradient scale, straight bf16 image, parked gradient pieces (AdamArgs::fold), fragment-order weight images (AdamArgs::frag) -- through
mimrl_op_adam_ex, and the fragment-image layout of mlp_fused.hip (frag_images_kernel) through mimrl_op_frag_images.

Reference: ONE NumPy routine (adam_ref) evaluates the kernel's formula in float64 on the fp32 inputs.  No tolerance constant is fixed here:
the same routine is also evaluated in float32, and the band of p, m and v is BAND_FACTOR = 8 x the largest |float32 - float64| of that array
(8: powf and FMA contraction on the device, which the float32 NumPy evaluation does not reproduce).  Everything else -- the bf16 images, the
fragment layout, the re-zeroed buffers, scalar against 8-wide kernel -- is compared bit for bit.

Measured with this file (n = 600 011, 6 steps, lr 4e-3 -> 2e-3, |p| <= 5, |m| <= 0.95, |v| <= 0.04): the float32-float64 gap of the reference
(the band is 8 x it) and the worst error of the MI355X against the float64 reference, per array:

  (wd, clip, gscale)     gap p    gap m    gap v     device p  device m  device v
  (0.01, 1.5,  1.0)      7.6e-7   1.2e-7   3.1e-9    7.6e-7    9.1e-8    2.3e-9
  (0,    0,    0.5)      6.8e-7   1.3e-7   5.4e-9    6.8e-7    9.2e-8    4.3e-9
  (0.01, 0.25, 0.125)    6.0e-6   2.5e-8   9.0e-11   9.8e-7    1.4e-8    7.3e-11

The parked-piece and 8-wide cases (1 and 2 steps) stay at or below 1.0 x their gap as well (p 1.9e-7 .. 4.2e-7, m <= 3.9e-8, v <= 8.8e-10);
every test prints its figures (`adam ...` lines) before it asserts.  The scalar and the 8-wide kernel agree bit for bit in p, m and v.
The largest case, (e), holds about 0.55 GB of device memory while both kernels' results are alive.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from mimrl_amd import _lib
from tests.gpu_helpers import P, dev, stream

pytestmark = pytest.mark.gpu

B1, B2, EPS = 0.9, 0.999, 1e-8
BAND_FACTOR = 8
SENTINEL = 0x7FC1          # a bf16 NaN pattern: no finite parameter rounds to it
N_SCALAR = 600011          # odd, > 2048 x 256 threads of the capped grid: every thread takes a second trip
SETTINGS = [(0.01, 1.5, 1.0), (0.0, 0.0, 0.5), (0.01, 0.25, 0.125)]      # (weight decay, clip, gradient scale)
# (OUT, RED, nb, gstride) of the fragment-image cases: every stride leaves a gap of non-matrix floats behind each matrix
SHAPES = [(32, 192, 3, 6184), (64, 128, 5, 8216), (96, 384, 7, 36872), (256, 256, 2, 197504)]


@pytest.fixture(scope="module")
def lib():
    lib = _lib.load()
    _lib.check(lib.mimrl_device_check())
    return lib


def adam_ref(dt, p, g, m, v, t, lr, wd, clip, gscale):
    """adam_kernel's formula in dtype ``dt`` on arrays of that dtype; the scalars are the fp32 values the kernel receives."""
    b1, b2, eps, lr, wd_, clip_, gs = (dt(np.float32(x)) for x in (B1, B2, EPS, lr, wd, clip, gscale))
    one = dt(1)
    bc1, bc2 = one - np.power(b1, dt(t)), one - np.power(b2, dt(t))
    step_size, inv_sqrt_bc2 = lr / bc1, one / np.sqrt(bc2)
    g = g * gs
    if clip > 0:
        g = np.minimum(np.maximum(g, -clip_), clip_)
    if wd != 0:
        g = g + wd_ * p
    m = b1 * m + (one - b1) * g
    v = b2 * v + (one - b2) * g * g
    p = p - step_size * m / (np.sqrt(v) * inv_sqrt_bc2 + eps)
    assert p.dtype == m.dtype == v.dtype == dt
    return p, m, v


class RefPair:
    """The float64 and the float32 trajectory of adam_ref from the same fp32 start."""

    def __init__(self, p, m, v):
        self.s = {dt: [np.asarray(x, np.float32).astype(dt) for x in (p, m, v)] for dt in (np.float64, np.float32)}

    def step(self, g, extra, t, lr, wd, clip, gscale):
        """g (+ extra, the parked pieces already scattered to bucket positions, or None): fp32 arrays."""
        for dt, (p, m, v) in self.s.items():
            gg = g.astype(dt) if extra is None else g.astype(dt) + extra.astype(dt)
            self.s[dt] = list(adam_ref(dt, p, gg, m, v, t, lr, wd, clip, gscale))

    def check(self, tag, p, m, v):
        """Device arrays within BAND_FACTOR x the float32-float64 gap of the reference; prints every figure before it asserts."""
        fails = []
        for name, got, want, w32 in zip("pmv", (p, m, v), self.s[np.float64], self.s[np.float32]):
            got = got.cpu().numpy()
            assert np.isfinite(got).all(), f"{tag}: non-finite {name}"
            gap = float(np.abs(w32.astype(np.float64) - want).max())
            err = float(np.abs(got.astype(np.float64) - want).max())
            print(f"adam {tag}: {name} float32-float64 gap {gap:.3e} on |values| <= {np.abs(want).max():.3g}, band {BAND_FACTOR * gap:.3e}, "
                  f"device error {err:.3e}")
            assert gap > 0, f"{tag}: the float32 evaluation of {name} equals the float64 one: no band"
            if err > BAND_FACTOR * gap:
                fails.append(f"{name}: {err:.3e} > {BAND_FACTOR * gap:.3e}")
        assert not fails, f"{tag}: " + "; ".join(fails)


def gradients(rng, n):
    """2 x normal; 1 in 97 exactly zero and another 1 in 97 of size 1e-6: the sign-like first steps, where a wrong eps placement shows."""
    g = (2 * rng.standard_normal(n)).astype(np.float32)
    i = np.arange(n)
    g[i % 97 == 0] = 0
    tiny = i % 97 == 1
    g[tiny] = (1e-6 * rng.standard_normal(int(tiny.sum()))).astype(np.float32)
    return g


def i32(xs):
    return (C.c_int32 * len(xs))(*[int(x) for x in xs])


def i64(xs):
    return (C.c_int64 * len(xs))(*[int(x) for x in xs])


def adam_ex(lib, p, g, m, v, n, lr, step, wd, clip, gscale, pimg=None, fold=(), frag=(), frag_dst=None):
    """fold: [(lo, rows, d, ld, src tensor)]; frag: [(off, OUT, RED, nb, gstride)].  -> return code"""
    fa = [None] * 5
    if fold:
        fa = [i64([f[0] for f in fold]), i32([f[1] for f in fold]), i32([f[2] for f in fold]), i32([f[3] for f in fold]),
              (C.c_void_p * len(fold))(*[f[4].data_ptr() for f in fold])]
    ga = [None] * 5
    if frag:
        ga = [i64([f[0] for f in frag]), i32([f[1] for f in frag]), i32([f[2] for f in frag]), i32([f[3] for f in frag]),
              i64([f[4] for f in frag])]
    return lib.mimrl_op_adam_ex(stream(), P(p), P(g), P(m), P(v), n, P(lr), P(step), B1, B2, EPS, wd, clip, gscale, P(pimg),
                                len(fold), *fa, len(frag), *ga, P(frag_dst))


def frag_images(lib, src, dst, entries):
    """entries: [(off, OUT, RED, nb, gstride, tr, dshift)]"""
    _lib.check(lib.mimrl_op_frag_images(stream(), P(src), P(dst), len(entries), i64([e[0] for e in entries]), i32([e[1] for e in entries]),
                                        i32([e[2] for e in entries]), i32([e[3] for e in entries]), i32([e[5] for e in entries]),
                                        i64([e[4] for e in entries]), i64([e[6] for e in entries])))


def image_source(entries, length):
    """The definition in the comment of frag_images_kernel as a gather index: inv[d] = the element of src whose bf16 value position d
    of the image holds, or -1 where the image is not written (int32 [length])."""
    inv = np.full(length, -1, np.int32)
    for off, OUT, RED, nb, gs, tr, dshift in entries:
        c, r = np.arange(OUT, dtype=np.int64)[:, None], np.arange(RED, dtype=np.int64)[None, :]
        pos = ((c // 32 * (RED // 16) + r // 16) * 64 + c % 32 + 32 * ((r % 16) // 8)) * 8 + r % 8
        elem = r * OUT + c if tr else c * RED + r
        base = off + gs * np.arange(nb, dtype=np.int64)[:, None]
        d = (dshift + base + pos.reshape(1, -1)).reshape(-1)
        assert d.min() >= 0 and d.max() < length and (inv[d] == -1).all() and len(np.unique(d)) == len(d), "the test's own table overlaps"
        inv[d] = (base + elem.reshape(1, -1)).reshape(-1)
    return inv


def expected_image(src, inv_dev):
    """bf16(src) permuted by image_source's index (on the device), the sentinel elsewhere: int16 bits."""
    bits = src.to(torch.bfloat16).view(torch.int16)
    out = bits.index_select(0, inv_dev.clamp(min=0))
    return torch.where(inv_dev >= 0, out, torch.full_like(out, sentinel_i16()))


def sentinel_i16():
    return int(np.array(SENTINEL, np.uint16).view(np.int16))


def sentinel_buffer(length):
    return torch.full((length,), sentinel_i16(), dtype=torch.int16, device="cuda")


def bf16_bits(t):
    return t.to(torch.bfloat16).view(torch.int16)


def lay_out(shapes, lead=8):
    """Forward entries one after another at offsets that are multiples of 8 -> (entries, bucket length, a multiple of 8)."""
    entries, off = [], lead
    for OUT, RED, nb, gs in shapes:
        assert off % 8 == 0 and gs % 8 == 0 and gs > OUT * RED
        entries.append((off, OUT, RED, nb, gs, 0, 0))
        off += nb * gs
    return entries, off


@pytest.mark.parametrize("wd,clip,gscale", SETTINGS)
def test_scalar_kernel_full_form(lib, wd, clip, gscale):
    """(a) adam_kernel over a bucket every thread loops on: 6 steps with the device step counter, lr rewritten on the device before
    step 4, weight decay / value clip / gradient scale, the straight bf16 image."""
    n = N_SCALAR
    rng = np.random.default_rng(11)
    p0 = rng.standard_normal(n).astype(np.float32)
    ref = RefPair(p0, np.zeros(n, np.float32), np.zeros(n, np.float32))
    p, m, v = dev(p0), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    pimg = sentinel_buffer(n)
    lr, step = dev(np.array([4e-3], np.float32)), torch.zeros(1, dtype=torch.int32, device="cuda")
    lr_host = 4e-3
    for t in range(1, 7):
        if t == 4:
            lr_host = 2e-3
            lr.fill_(lr_host)
        step += 1
        gr = gradients(rng, n)
        g = dev(gr)
        _lib.check(adam_ex(lib, p, g, m, v, n, lr, step, wd, clip, gscale, pimg=pimg))
        torch.cuda.synchronize()
        ref.step(gr, None, t, lr_host, wd, clip, gscale)
        assert not g.any(), f"step {t}: the gradient bucket is not left zero"
        assert torch.equal(pimg, bf16_bits(p)), f"step {t}: the bf16 image is not bf16(p)"
    ref.check(f"scalar wd={wd} clip={clip} gscale={gscale}", p, m, v)


def test_parked_pieces_are_added_and_rezeroed(lib):
    """(b) AdamArgs::fold at the struct's capacity: 8 pieces of 12 rows with the pads of d_v = 35 (48), d_a = 74 (80) and no pad (128); one
    adjacent pair, one piece across index 524 288 (the second trip of the grid-stride loop), unaligned starts, the table out of order so
    that lo_all / hi_all are a real min / max.  The padding columns hold NaN (then 7.0): they belong to no parameter and must come back zero.
    Weight decay 0.01, clip 1.5 (wide enough that few of the sums clip: a clipped element hides its parked piece), gradient scale 0.5."""
    n = N_SCALAR
    wd, clip, gscale = 0.01, 1.5, 0.5
    shapes = [(35, 48), (74, 80), (128, 128)]
    los = [523788, 1003, 1423, 599123, 40000, 100001, 200000, 300007]       # 1003 + 12 * 35 = 1423: adjacent; 599123 + 12 * 74 = n
    dl = [shapes[2], shapes[0], shapes[1], shapes[1], shapes[0], shapes[1], shapes[2], shapes[0]]
    rows = 12
    assert los[1] + rows * dl[1][0] == los[2] and los[0] < 524288 < los[0] + rows * dl[0][0] and los[3] + rows * dl[3][0] == n
    rng = np.random.default_rng(12)
    p0 = rng.standard_normal(n).astype(np.float32)
    ref = RefPair(p0, np.zeros(n, np.float32), np.zeros(n, np.float32))
    p, m, v = dev(p0), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    lr, step = dev(np.array([4e-3], np.float32)), torch.zeros(1, dtype=torch.int32, device="cuda")
    for t, pad in ((1, np.nan), (2, 7.0)):
        step += 1
        gr = gradients(rng, n)
        extra = np.zeros(n, np.float32)
        fold = []
        for lo, (d, ld) in zip(los, dl):
            s = np.full((rows, ld), pad, np.float32)
            s[:, :d] = rng.standard_normal((rows, d)).astype(np.float32)
            extra[lo:lo + rows * d] = s[:, :d].reshape(-1)
            fold.append((lo, rows, d, ld, dev(s)))
        g = dev(gr)
        _lib.check(adam_ex(lib, p, g, m, v, n, lr, step, wd, clip, gscale, fold=fold))
        torch.cuda.synchronize()
        ref.step(gr, extra, t, 4e-3, wd, clip, gscale)
        ref.check(f"fold call {t}", p, m, v)
        assert not g.any(), f"call {t}: the gradient bucket is not left zero"
        for q, f in enumerate(fold):
            assert torch.equal(f[4], torch.zeros_like(f[4])), f"call {t}: parked piece {q} (d {f[2]}, ld {f[3]}) is not left entirely zero"


def test_fragment_image_layout_matches_its_definition(lib):
    """(c) frag_images_kernel against the definition in its comment: forward entries of every shape, and two of them again as the
    data-gradient image (tr = 1) one buffer length further on, as the engine lays them out."""
    fwd, n = lay_out(SHAPES)
    entries = fwd + [(e[0], e[1], e[2], e[3], e[4], 1, n) for e in (fwd[1], fwd[3])]
    src = dev(np.random.default_rng(13).standard_normal(n).astype(np.float32))
    dst = sentinel_buffer(2 * n)
    frag_images(lib, src, dst, entries)
    torch.cuda.synchronize()
    inv = image_source(entries, 2 * n)
    covered = int((inv >= 0).sum())
    assert covered == sum(e[1] * e[2] * e[3] for e in entries) and covered < 2 * n
    want = expected_image(src, torch.from_numpy(inv).cuda())
    bad = (dst != want).nonzero().flatten()
    assert bad.numel() == 0, f"{bad.numel()} image positions differ, first at {int(bad[0])} (source element {int(inv[int(bad[0])])}; -1 = sentinel)"


def _eight_wide_against_scalar(lib, n, frag_entries, p0, m0, v0, grads, wd, clip, gscale, ref=None):
    """adam8_kernel with images against adam_kernel on copies, frag_images_kernel and the NumPy permutation: the checks of (d)."""
    frag = [e[:5] for e in frag_entries]
    inv = torch.from_numpy(image_source(frag_entries, n)).cuda()
    lr = dev(np.array([4e-3], np.float32))
    step = torch.zeros(1, dtype=torch.int32, device="cuda")
    ps, ms, vs = dev(p0), dev(m0), dev(v0)             # the scalar kernel's copies
    p8, m8, v8 = dev(p0), dev(m0), dev(v0)
    pimg, fimg = sentinel_buffer(n), sentinel_buffer(n)
    for t, gr in enumerate(grads, 1):
        step += 1
        g = dev(gr)
        _lib.check(adam_ex(lib, ps, g, ms, vs, n, lr, step, wd, clip, gscale))
        del g
        g = dev(gr)
        _lib.check(adam_ex(lib, p8, g, m8, v8, n, lr, step, wd, clip, gscale, pimg=pimg, frag=frag, frag_dst=fimg))
        torch.cuda.synchronize()
        if ref is not None:
            ref.step(gr, None, t, 4e-3, wd, clip, gscale)
            ref.check(f"8-wide step {t}", p8, m8, v8)
        for name, a, b in (("p", p8, ps), ("m", m8, ms), ("v", v8, vs)):
            assert torch.equal(a, b), f"step {t}: {name} of the 8-wide kernel differs from the scalar kernel's in {int((a != b).sum())} elements"
        assert not g.any(), f"step {t}: the gradient bucket is not left zero"
        del g, a, b
        if t == len(grads):
            ps = ms = vs = None                        # (the large case: release the scalar kernel's copies before the image checks)
        assert torch.equal(pimg, bf16_bits(p8)), f"step {t}: the bf16 image is not bf16(p)"
        side = sentinel_buffer(n)
        frag_images(lib, p8, side, frag_entries)
        torch.cuda.synchronize()
        assert torch.equal(fimg, side), f"step {t}: the update's fragment images differ from frag_images_kernel's in {int((fimg != side).sum())} positions"
        del side
        want = expected_image(p8, inv)
        bad = (fimg != want).nonzero().flatten()
        assert bad.numel() == 0, f"step {t}: {bad.numel()} image positions differ from the definition, first at {int(bad[0])}"
        del want, bad


def test_eight_wide_kernel_with_images(lib):
    """(d) adam8_kernel writing the straight and the fragment-order images, two consecutive steps."""
    entries, n = lay_out(SHAPES)
    assert n % 8 == 0
    rng = np.random.default_rng(14)
    p0 = rng.standard_normal(n).astype(np.float32)
    z = np.zeros(n, np.float32)
    grads = [gradients(rng, n), gradients(rng, n)]
    _eight_wide_against_scalar(lib, n, entries, p0, z, z, grads, 0.01, 1.5, 0.5, ref=RefPair(p0, z, z))


def test_eight_wide_index_arithmetic_at_its_documented_bound(lib):
    """(e) "exact below 2^24 elements": 8160 matrices [32 x 64] 2056 apart fill a bucket of 16 776 960 floats -- group quotients up to 8159,
    n / 8 four times the capped grid.  One step from a state with non-zero moments; bit-equality checks only."""
    OUT, RED, nb, gs = 32, 64, 8160, 2056
    n = nb * gs
    assert n == 16776960 and n < 1 << 24 and n % 8 == 0
    rng = np.random.default_rng(15)
    p0 = rng.standard_normal(n, dtype=np.float32)
    m0 = 0.3 * rng.standard_normal(n, dtype=np.float32)
    v0 = 0.01 * rng.random(n, dtype=np.float32)
    gr = 2 * rng.standard_normal(n, dtype=np.float32)
    _eight_wide_against_scalar(lib, n, [(0, OUT, RED, nb, gs, 0, 0)], p0, m0, v0, [gr], 0.01, 1.5, 0.5)


def test_refusals_come_before_any_launch(lib):
    """(f) what the 8-wide kernel cannot do is refused with a negative code and a message, and nothing is launched: the gradient
    bucket, which every launch zeroes, keeps its values."""
    one = (0, 32, 64, 1, 2048)

    def refused(n, alloc, fold=(), frag=(one,)):
        p, m, v = (torch.zeros(alloc, device="cuda") for _ in range(3))
        g = torch.ones(alloc, device="cuda")
        lr, step = dev(np.array([4e-3], np.float32)), torch.ones(1, dtype=torch.int32, device="cuda")
        fimg = sentinel_buffer(alloc)
        rc = adam_ex(lib, p, g, m, v, n, lr, step, 0.01, 1.5, 1.0, fold=fold, frag=frag, frag_dst=fimg)
        torch.cuda.synchronize()
        msg = lib.mimrl_last_error().decode()
        assert rc < 0 and msg, (n, rc, msg)
        assert bool((g == 1).all()) and not p.any() and bool((fimg == sentinel_i16()).all()), f"n = {n}: refused, yet something ran"
        return msg

    refused(4099, 4104)                                                              # n % 8 != 0
    refused(4096, 4096, fold=[(2048, 12, 35, 48, torch.zeros(12, 48, device="cuda"))])   # images and parked pieces together
    refused(13 * 2048, 13 * 2048, frag=[(2048 * e, 32, 64, 1, 2048) for e in range(13)])   # 13 entries
    refused(1 << 24, 1 << 24, frag=[(0, 32, 64, 8, 2056)])                           # n = 2^24: buffers really that long
