"""Cases, yardsticks and bounds for the flow core: Farnebaeck's front end (blur, polynomial expansion, pyramid resize), the
cv2-style remap behind warp_flow / smooth_flow_step, and two identities of the variational refinement.

The kernels of these stages are compared bit for bit with their C twins (oracle/c/farneback.c, remap.c, varref.c).  Twin and
kernel have one author, so that comparison cannot see a weight, border rule or channel that both got wrong.  A yardstick here
states a stage as mathematics in float64 -- plus the few conventions of OpenCV that are definitions, named where they are
used -- and shares no expression with the twin.  mpmath (40 digits) is used for the 6 x 6 solve of the expansion and for the
weight tables, nothing else.

Every bound is  u * sum_k d_k |c_k| |f_k|  with u = 2^-24 (the unit roundoff of float32), c_k the yardstick's own coefficient
of input value f_k, and d_k the number of float32 roundings the term c_k f_k passes on its way through the stage (Higham,
Accuracy and Stability, section 3.1, to first order in u; a partial sum is bounded by the sum of the absolute terms, so a
rounding of a partial sum counts once for every term already in it).  Steps carried out in double contribute 2^-53 per step
and are not counted; neither is the yardstick's own float64 arithmetic.  K, the figure recorded in
profiles/flow_yardsticks.txt, is max_k d_k.  No bound holds a margin fitted to what the code returns: test_flow_yardsticks_cpu
asserts that the twin uses between 1/16 and all of each bound, so a bound cannot be a formality either.

1. Full-resolution blur.  The uint8 frame correlated with [1/4, 1/2, 1/4] in both axes, border reflect-101 (index -1 reads
   1, index n reads n - 2; a single row or column reads itself).  Every product and sum is a multiple of 1/16 below 2^8: exact
   in float32, so the requirement is equality.

2. Polynomial expansion (n, sigma).  At each pixel the weighted least-squares fit of  c + r_x x + r_y y + r_xx x^2 + r_yy y^2
   + r_xy x y  over the (2n + 1)^2 window, weights g(dx) g(dy), g ~ exp(-t^2 / 2 sigma^2) normalised to unit sum, the image
   extended by edge replication.  With b = (1, x, y, x^2, y^2, xy) and G = sum_w b b^T the coefficients are G^-1 sum_w b f: a
   6 x (2n + 1)^2 matrix C, built once.  The five output channels are (r_y, r_x, r_yy, r_xx, r_xy), in that order.
   Roundings of a term: the twin's 1-D tables are g = fl(fl(e) / S) (2; the error of S is common to all taps and leaves a
   least-squares fit unchanged), xg = fl(x g) and xxg = fl(x^2 g) (3 each); a term carries one vertical and one horizontal
   table entry: 6.  The vertical pass is float32: the pair sum fl(s0 + s1), the product, and the n - k + 1 additions that
   follow tap k: at most n + 2 (the centre tap: one product, n additions).  The horizontal pass and the products with inv(G)
   are in double.  One final cast.  K = 6 + (n + 2) + 1 = n + 9: 14 for n = 5, 16 for n = 7.
   The count treats the twin's table error as an error of the term.  (The twin inverts the G of its own rounded g, so the
   part of it that comes from g is a perturbation of the fit's weights and acts on the residual of the fit rather than on f;
   to first order that is no larger.)  r_xx and r_yy are formed as b1 ig03 + b4 ig33 with ig03 < 0 < ig33: where the two
   nearly cancel (x^2 = 1 at sigma 1.1) one tap's error can exceed K u |c_k| |f_k|; the bound is on the window's sum.

3. Pyramid blur (ksize, sigma > 0).  Correlation with k ~ exp(-t^2 / 2 sigma^2) / sum in both axes, reflect-101.
   Roundings of a term: a 1-D table entry is fl(fl(e) / S') with S' the double sum of the rounded fl(e): numerator, denominator
   and cast, 3 per axis.  Row pass (ksize > 5: one product per tap, added left to right): tap j passes 1 + (ksize - max(j,
   1)) roundings; ksize = 3: S k1 + (S- + S+) k0: 2 for the centre, 3 for the pair.  Column pass (symmetric): the pair sum,
   the product and the r - i + 1 additions after pair i; the centre one product and r additions.  d = 6 + row + column is
   kept per tap; K = 6 + ksize + (r + 2) (12 at ksize 3) is its maximum.

4. Resize.  Exact 2 x decimation: the mean of the 2 x 2 block, ((a + b) + c) + d in float32, then a scaling by 1/4 that is
   exact: d = (3, 3, 2, 1), K = 3.  Otherwise bilinear at the source coordinate s = (dst + 1/2) scale - 1/2 (pixel centres),
   i = floor(s), t = s - i; in x an index below 0 or from n - 1 on reads that edge pixel alone, in y the two row indices are
   clamped (the same values).  The twin forms s in double and casts it to float32: s moves by at most u |s|, and the result
   by  u |s_x| |d/dx| + u |s_y| |d/dy|  with |d/dx| <= (1 - t_y) |f01 - f00| + t_y |f11 - f10| and likewise in y: the
   coordinate term.  (t = fl(s) - i is then exact.)  Arithmetic term: the weight 1 - t is rounded (1), t is not; per axis
   one product and one addition: d = 4 + [x weight is 1 - t] + [y weight is 1 - t], K = 6.  The case set keeps every s that
   float32 does not hold exactly further than 2^-20 max(1, |s|) from an integer (asserted), so floor() agrees.

5. Remap (linear, cubic, Lanczos-4).  Definitions: the sample coordinate is fl32(x + u), fl32(y + v); it is quantised to
   q = rint(32 coord) / 32, ties to even; the footprint is 2 x 2, 4 x 4 or 8 x 8 anchored at floor(q) - {0, 1, 3}; every tap
   of the footprint counts, even at weight zero, and with a NaN border a tap outside the image makes the result NaN.  1-D
   weights at t = q - floor(q): the hat function; Keys' cubic with a = -0.75; sinc(z) sinc(z / 4) normalised to unit sum over
   the eight taps (a delta at t = 0).  The 2-D weight is the product.
   Weight error.  Linear: t and 1 - t are multiples of 1/32, their products exact: 0.  Cubic: Horner's scheme in float32 on
   multiples of 1/32 with coefficients that are multiples of 1/4 never needs more than 2^-17 below a magnitude of 16, so the
   1-D weights are exact, and the 2-D product (34 bits) rounds once: relative u.  Lanczos-4: a 1-D entry is
   fl(fl(e_i) * fl(1 / S)), S the float32 sum of the eight fl(e_i) from left to right.  S is off by at most u (sum_i |w_i| +
   sum_{k >= 2} |s_k|) relative to sum w = 1 (the casts; the seven additions, s_k the partial sums), the reciprocal by u, the
   entry's own cast and product 2 u: e(t) = 3 + sum |w_i| + sum_{k >= 2} |s_k|, evaluated on the yardstick's own table (at
   most 9.56, at t = 11/32); the 2-D product e(t_y) + e(t_x) + 1.  All of it is relative to |w|: in the form
   u (K_w sum_footprint |f| + K_s sum |w| |f|) K_w = 0 for all three methods.
   Summation.  Linear: ((p0 + p1) + p2) + p3: d = (4, 4, 3, 2).  Cubic: 16 products added left to right, row-major: tap q
   passes 1 + 16 - max(q, 1).  Lanczos-4: each row's 8 products left to right, the row sums added top to bottom to a zero:
   1 + (8 - max(j, 1)) + (8 - max(r, 1)).  K_s = weight error + summation at its maximum: 4, 17, 15 + 2 * 9.56 + 1 < 36.
   smooth_flow_step: f' = (f - warp(b by f)) / 2 per component where the warp is finite, f where it is NaN: half the warp's
   bound plus one rounding of the sum.

6. Refinement.  Two identities that hold exactly: identical frames with a zero flow return zeros; constant frames with a
   constant flow return the flow's bits.  (The analogous identity does NOT hold for Farnebaeck: DESIGN.md section 2.)
"""
import functools

import numpy as np

U = 2.0 ** -24
DEFAULT_POLY = (5, 1.1)
OTHER_POLY = (7, 1.5)

# ---- cases ----------------------------------------------------------------------------------------------------------------
# expansion: the issue's shapes; 21 x 70 has a second tile row (16 rows per tile) that holds two of the kernel's four-row
# groups, the last one cut, and a second tile column (64); 96 x 128 is six by two full tiles
EXPANSION_SHAPES = ((1, 1), (1, 9), (7, 1), (7, 5), (12, 14), (17, 65), (40, 50), (96, 128), (21, 70))
EXPANSION_CONTENTS = ("noise", "checker", "constant")
# x^2 + y^2 - x y + 2 x + 3 y + 60 about the pixel (x, y) = (7, 6): integers within 54 .. 214 on 14 x 16
QUADRATIC = dict(c=60.0, x=2.0, y=3.0, xx=1.0, yy=1.0, xy=-1.0, x0=7.0, y0=6.0)
QUADRATIC_SHAPE = (14, 16)
PYRAMID_LEVELS = (1, 2, 3, 4)
BLUR_SHAPES = ((1, 1), (5, 7), (40, 50), (61, 83))                           # smaller than every kernel ... larger than all but 39
# (source, destination, channels): halvings, odd sizes, the 4 x and 8 x steps of levels 2 and 3, the flow's upsampling
RESIZE_HALVINGS = (((2, 2), (1, 1), 1), ((40, 50), (20, 25), 1), ((96, 128), (48, 64), 2))
RESIZE_BILINEAR = (((333, 37), (166, 18), 1), ((41, 333), (20, 166), 1), ((160, 200), (40, 50), 1), ((96, 128), (12, 16), 1),
                   ((20, 25), (40, 50), 2), ((21, 32), (41, 63), 2), ((5, 7), (9, 13), 2), ((3, 1), (5, 1), 1))
REMAP_METHODS = ("linear", "cubic", "lanczos")
REMAP_SHAPES = ((1, 1), (2, 3), (3, 9), (7, 7), (37, 53), (9, 130))          # 130 > 2 * 64: three workgroups of k_warp across
REMAP_FLOWS = ("amp0.3", "amp6", "amp80", "ties", "last")
VARREF_TW, VARREF_TH = 128, 8                                                # as tests/test_gpu_varref_sources.py names them
VARREF_SHAPES = ((1, 1), (2, 3), (7, 9), (VARREF_TH + 1, VARREF_TW + 1), (2 * VARREF_TH + 1, 2 * VARREF_TW + 3))
VARREF_CONSTANT_FLOW = (0.3125, -1.7)


def _seed(*key):
    return sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31)


def frame(shape, content, seed=0):
    """uint8 frame: smoothed noise stretched to 0 .. 255, a 0 / 255 checkerboard, or a constant grey"""
    import scipy.ndimage as ndi
    h, w = shape
    if content == "checker":
        yy, xx = np.mgrid[0:h, 0:w]
        return (((yy + xx) & 1) * 255).astype(np.uint8)
    if content == "constant":
        return np.full(shape, 93, np.uint8)
    a = ndi.gaussian_filter(np.random.default_rng(_seed(h, w, seed)).normal(size=(h + 8, w + 8)), 2.0)[4:-4, 4:-4]
    return np.ascontiguousarray(((a - a.min()) / (np.ptp(a) + 1e-9) * 255).astype(np.uint8))


def quadratic_frame(shape=QUADRATIC_SHAPE, q=QUADRATIC):
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]].astype(np.float64)
    xx, yy = xx - q["x0"], yy - q["y0"]
    return q["c"] + q["x"] * xx + q["y"] * yy + q["xx"] * xx * xx + q["yy"] * yy * yy + q["xy"] * xx * yy


def quadratic_coefficients(shape=QUADRATIC_SHAPE, q=QUADRATIC):
    """the local expansion of the quadratic about every pixel, in the output's channel order (r_y, r_x, r_yy, r_xx, r_xy)"""
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]].astype(np.float64)
    xx, yy = xx - q["x0"], yy - q["y0"]
    one = np.ones(shape)
    return np.stack([q["y"] + 2 * q["yy"] * yy + q["xy"] * xx, q["x"] + 2 * q["xx"] * xx + q["xy"] * yy,
                     q["yy"] * one, q["xx"] * one, q["xy"] * one], -1)


def remap_image(shape, seed=0):
    rng = np.random.default_rng(_seed(shape[0], shape[1], seed, 17))
    return (rng.normal(size=shape) * 40.0 + 250.0).astype(np.float32)


def remap_flow(shape, kind, seed=0):
    """(h, w, 2) float32 flow (u, v).  amp*: white noise of that amplitude with a few vectors far out; ties: every component an
    odd multiple of 1/64, so 32 * coordinate ends in .5 and round-half-even decides, up as often as down; last: integer
    coordinates on the last column, the last row, the last pixel, one column beyond, and -- as controls -- the pixel's own place
    and the last place whose 2 x 2 footprint lies inside."""
    h, w = shape
    rng = np.random.default_rng(_seed(h, w, seed, sum(map(ord, kind))))
    if kind.startswith("amp"):
        amp = float(kind[3:])
        f = (rng.uniform(-amp, amp, size=shape + (2,))).astype(np.float32)
        f[rng.random(shape) < 0.03] = np.float32(amp * 3 + 5)
        return f
    if kind == "ties":
        return ((rng.integers(-3 * 64, 3 * 64, size=shape + (2,)) | 1) / 64.0).astype(np.float32)
    assert kind == "last"
    yy, xx = np.mgrid[0:h, 0:w]
    which = (yy + 2 * xx) % 6              # 4: stays where it is; 5: the last place whose 2 x 2 footprint is inside
    f = np.zeros(shape + (2,), np.float32)
    f[..., 0] = np.select([which == 3, which == 5, (which == 0) | (which == 2)], [w - xx, max(w - 2, 0) - xx, (w - 1) - xx], 0)
    f[..., 1] = np.select([which == 5, (which == 1) | (which == 2)], [max(h - 2, 0) - yy, (h - 1) - yy], 0)
    return f


# ---- shared pieces --------------------------------------------------------------------------------------------------------
def reflect101(idx, n):
    """index map of BORDER_REFLECT_101, applied until the index is inside (windows wider than the image)"""
    idx = np.asarray(idx).copy()
    if n == 1:
        return np.zeros_like(idx)
    for _ in range(64):
        idx = np.where(idx < 0, -idx, idx)
        idx = np.where(idx >= n, 2 * n - 2 - idx, idx)
        if ((idx >= 0) & (idx < n)).all():
            return idx
    raise AssertionError("reflect101 did not settle")


def _sep_corr(img, ky, kx, border):
    """sum_ij ky[i] kx[j] img[b(y + i - ry), b(x + j - rx)] in float64; border: index map (idx, n) -> idx"""
    img = np.asarray(img, np.float64)
    h, w = img.shape
    ry, rx = len(ky) // 2, len(kx) // 2
    tmp = np.zeros((h, w))
    for j, c in enumerate(kx):
        tmp += c * img[:, border(np.arange(w) + j - rx, w)]
    out = np.zeros((h, w))
    for i, c in enumerate(ky):
        out += c * tmp[border(np.arange(h) + i - ry, h)]
    return out


# ---- 1. the full-resolution blur ------------------------------------------------------------------------------------------
def blur3_yardstick(img_u8):
    k = np.array([0.25, 0.5, 0.25])
    return _sep_corr(img_u8, k, k, reflect101)


# ---- 2. polynomial expansion ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def expansion_matrix(n, sigma, border="replicate"):
    """C (5, 2n + 1, 2n + 1): output channel, dy, dx.  The normal equations in mpmath at 40 digits."""
    import mpmath as mp
    with mp.workdps(40):
        g = [mp.exp(-mp.mpf(t) ** 2 / (2 * mp.mpf(sigma) ** 2)) for t in range(-n, n + 1)]
        s = mp.fsum(g)
        g = [v / s for v in g]
        basis = lambda x, y: [mp.mpf(1), mp.mpf(x), mp.mpf(y), mp.mpf(x * x), mp.mpf(y * y), mp.mpf(x * y)]   # noqa: E731
        G = mp.zeros(6, 6)
        for iy, y in enumerate(range(-n, n + 1)):
            for ix, x in enumerate(range(-n, n + 1)):
                b = basis(x, y)
                wgt = g[iy] * g[ix]
                for a in range(6):
                    for c in range(6):
                        G[a, c] += wgt * b[a] * b[c]
        Gi = mp.inverse(G)                                                      # the 6 x 6 solve
        C = np.zeros((6, 2 * n + 1, 2 * n + 1))
        for iy, y in enumerate(range(-n, n + 1)):
            for ix, x in enumerate(range(-n, n + 1)):
                b = basis(x, y)
                wgt = g[iy] * g[ix]
                for a in range(6):
                    C[a, iy, ix] = float(mp.fsum(Gi[a, c] * b[c] for c in range(6)) * wgt)
    return np.ascontiguousarray(C[[2, 1, 4, 3, 5]])                             # (r_y, r_x, r_yy, r_xx, r_xy)


def expansion_K(n):
    return n + 9


def _windows(img, n, border):
    img = np.asarray(img, np.float64)
    h, w = img.shape
    if border == "replicate":
        iy, ix = np.clip(np.arange(-n, h + n), 0, h - 1), np.clip(np.arange(-n, w + n), 0, w - 1)
    else:
        iy, ix = reflect101(np.arange(-n, h + n), h), reflect101(np.arange(-n, w + n), w)
    pad = img[np.ix_(iy, ix)]
    return np.lib.stride_tricks.sliding_window_view(pad, (2 * n + 1, 2 * n + 1))


def expansion_yardstick(blurred, n=5, sigma=1.1, border="replicate"):
    """(value, bound), both (h, w, 5) float64.  border="reflect" states the WRONG border on purpose (sensitivity tests, which
    take their bound from the right statement)."""
    C = expansion_matrix(n, float(sigma))
    win = _windows(blurred, n, border)
    value = np.einsum("cij,yxij->yxc", C, win, optimize=True)
    bound = expansion_K(n) * U * np.einsum("cij,yxij->yxc", np.abs(C), np.abs(win), optimize=True)
    return value, bound


# ---- 3. the pyramid's blur ------------------------------------------------------------------------------------------------
def pyramid_blur_params(level):
    sigma = (2 ** level - 1) / 2.0
    ksize = max(int(np.rint(sigma * 5)) | 1, 3)                                 # rint: ties to even, as cvRound
    return ksize, sigma


@functools.lru_cache(maxsize=None)
def gaussian_taps(ksize, sigma):
    import mpmath as mp
    with mp.workdps(40):
        r = ksize // 2
        e = [mp.exp(-mp.mpf(t) ** 2 / (2 * mp.mpf(sigma) ** 2)) for t in range(-r, r + 1)]
        s = mp.fsum(e)
        return np.array([float(v / s) for v in e])


def blur_depths(ksize):
    """roundings of a term by tap: (row pass by j, column pass by i), the table's 3 + 3 not included"""
    r = ksize // 2
    j = np.arange(ksize)
    if ksize == 3:
        row = np.array([3.0, 2.0, 3.0])
    elif ksize == 5:
        row = np.array([3.0, 4.0, 3.0, 4.0, 3.0])
    else:
        row = 1.0 + ksize - np.maximum(j, 1)
    d = np.abs(j - r)
    col = np.where(d == 0, 1.0 + r, 2.0 + r - d + 1.0)
    return row, col


def blur_K(ksize):
    row, col = blur_depths(ksize)
    return int(6 + row.max() + col.max())


def blur_yardstick(img, ksize, sigma):
    k = gaussian_taps(ksize, float(sigma))
    row, col = blur_depths(ksize)
    a = np.abs(np.asarray(img, np.float64))
    value = _sep_corr(img, k, k, reflect101)
    bound = U * (6 * _sep_corr(a, k, k, reflect101) + _sep_corr(a, k, k * row, reflect101) + _sep_corr(a, k * col, k, reflect101))
    return value, bound


# ---- 4. resize ------------------------------------------------------------------------------------------------------------
RESIZE_K_MEAN, RESIZE_K_BILINEAR = 3, 6


def halving_yardstick(src):
    """src (h, w, cn) with even h, w -> (value, bound) of the 2 x 2 mean"""
    s = np.asarray(src, np.float64)
    a, b, c, d = s[0::2, 0::2], s[0::2, 1::2], s[1::2, 0::2], s[1::2, 1::2]
    return (a + b + c + d) / 4, U * (3 * np.abs(a) + 3 * np.abs(b) + 2 * np.abs(c) + np.abs(d)) / 4


def _resize_axis(dn, sn, corner=False):
    scale = sn / dn
    s = np.arange(dn) * scale if corner else (np.arange(dn) + 0.5) * scale - 0.5
    i = np.floor(s).astype(np.int64)
    t = s - i
    inexact = s != s.astype(np.float32).astype(np.float64)
    gap = np.abs(s - np.rint(s))
    assert (gap[inexact] > 2.0 ** -20 * np.maximum(1, np.abs(s[inexact]))).all(), "a coordinate too near an integer for this case set"
    out = (i < 0) | (i >= sn - 1)
    t = np.where(out, 0.0, t)
    i0 = np.clip(i, 0, sn - 1)
    i1 = np.where(out, i0, np.clip(i + 1, 0, sn - 1))
    return i0, i1, t, np.where(out, 0.0, np.abs(s))


def bilinear_yardstick(src, dshape, corner=False):
    """src (sh, sw, cn) -> (value, bound) at (dh, dw, cn); corner=True states the pixel-corner convention (sensitivity test)"""
    s = np.asarray(src, np.float64)
    sh, sw = s.shape[:2]
    y0, y1, ty, cy = _resize_axis(dshape[0], sh, corner)
    x0, x1, tx, cx = _resize_axis(dshape[1], sw, corner)
    ty, cy = ty[:, None, None], cy[:, None, None]
    tx, cx = tx[None, :, None], cx[None, :, None]
    f00, f01, f10, f11 = s[np.ix_(y0, x0)], s[np.ix_(y0, x1)], s[np.ix_(y1, x0)], s[np.ix_(y1, x1)]
    value = (1 - ty) * ((1 - tx) * f00 + tx * f01) + ty * ((1 - tx) * f10 + tx * f11)
    arith = ((1 - ty) * (1 - tx) * 6 * np.abs(f00) + (1 - ty) * tx * 5 * np.abs(f01) + ty * (1 - tx) * 5 * np.abs(f10)
             + ty * tx * 4 * np.abs(f11))
    coord = (cx * ((1 - ty) * np.abs(f01 - f00) + ty * np.abs(f11 - f10))
             + cy * ((1 - tx) * np.abs(f10 - f00) + tx * np.abs(f11 - f01)))
    return value, U * (arith + coord)


# ---- 5. remap -------------------------------------------------------------------------------------------------------------
REMAP_TAPS = {"linear": 2, "cubic": 4, "lanczos": 8}
REMAP_ANCHOR = {"linear": 0, "cubic": 1, "lanczos": 3}


@functools.lru_cache(maxsize=None)
def remap_table(method, a=-0.75, bins=32):
    """(bins, taps) float64 1-D weights at t = k / bins"""
    import mpmath as mp
    taps, anchor = REMAP_TAPS[method], REMAP_ANCHOR[method]
    out = np.zeros((bins, taps))
    with mp.workdps(40):
        A = mp.mpf(a)
        for k in range(bins):
            t = mp.mpf(k) / bins
            row = []
            for i in range(taps):
                z = abs(t - (i - anchor))                                        # distance of tap i from the sample point
                if method == "linear":
                    row.append(max(mp.mpf(0), 1 - z))
                elif method == "cubic":
                    row.append((A + 2) * z ** 3 - (A + 3) * z ** 2 + 1 if z <= 1 else
                               (A * z ** 3 - 5 * A * z ** 2 + 8 * A * z - 4 * A if z < 2 else mp.mpf(0)))
                else:
                    row.append(mp.sincpi(z) * mp.sincpi(z / 4) if z < 4 else mp.mpf(0))
            if method == "lanczos":
                s = mp.fsum(row)
                row = [v / s for v in row]
            out[k] = [float(v) for v in row]
    return out


@functools.lru_cache(maxsize=None)
def remap_weight_error(method):
    """relative error of a 1-D table entry by phase, in units of u (docstring, 5.)"""
    tab = remap_table(method)
    if method != "lanczos":
        return np.zeros(len(tab))
    e = 3.0 + np.abs(tab).sum(1) + np.abs(np.cumsum(tab, 1))[:, 1:].sum(1)
    e[0] = 0.0                                                                  # the delta at t = 0 is exact
    return e


@functools.lru_cache(maxsize=None)
def remap_depths(method):
    """(taps, taps) roundings of a term in the summation, the product included"""
    n = REMAP_TAPS[method]
    if method == "linear":
        return np.array([[4.0, 4.0], [3.0, 2.0]])
    r, j = np.mgrid[0:n, 0:n]
    if method == "cubic":
        return 1.0 + 16 - np.maximum(r * 4 + j, 1)
    return 1.0 + (8 - np.maximum(j, 1)) + (8 - np.maximum(r, 1))


def remap_K(method):
    e = remap_weight_error(method).max()
    return float(remap_depths(method).max() + (0 if method == "linear" else 1 if method == "cubic" else 2 * e + 1))


def remap_yardstick(img, flow, method, a=-0.75, bins=32, quantise="rint"):
    """img (h, w) float32, flow (h, w, 2) float32 -> (value with NaN where a tap of the footprint is outside, bound).  `a`,
    `bins`, `quantise` other than the defaults state the WRONG convention on purpose (sensitivity tests, which take their
    bound from the right statement)."""
    img64 = np.asarray(img, np.float64)
    h, w = img64.shape
    yy, xx = np.mgrid[0:h, 0:w]
    mx = (xx.astype(np.float32) + flow[..., 0].astype(np.float32)).astype(np.float64)    # fl32(x + u)
    my = (yy.astype(np.float32) + flow[..., 1].astype(np.float32)).astype(np.float64)
    rnd = np.rint if quantise == "rint" else np.trunc
    fx, fy = rnd(mx * bins).astype(np.int64), rnd(my * bins).astype(np.int64)
    sx, sy = np.floor_divide(fx, bins), np.floor_divide(fy, bins)
    kx, ky = fx - sx * bins, fy - sy * bins
    taps, anchor = REMAP_TAPS[method], REMAP_ANCHOR[method]
    tab = remap_table(method, a, bins)
    err = remap_weight_error(method) if bins == 32 else np.zeros(bins)
    depth = remap_depths(method)
    extra = {"linear": 0.0, "cubic": 1.0, "lanczos": 1.0}[method]
    bx, by = sx - anchor, sy - anchor
    inside = (bx >= 0) & (bx + taps <= w) & (by >= 0) & (by + taps <= h)
    value, bound = np.zeros((h, w)), np.zeros((h, w))
    for r in range(taps):
        for j in range(taps):
            term = tab[ky, r] * tab[kx, j] * img64[np.clip(by + r, 0, h - 1), np.clip(bx + j, 0, w - 1)]
            value += term
            bound += (depth[r, j] + err[ky] + err[kx] + extra) * np.abs(term)
    value[~inside] = np.nan
    return value, U * bound


def smooth_step_yardstick(fwd, bwd, method):
    """((f', bound), (b', bound)) of smooth_flow_step in float64"""
    def half(f, other):
        out, bnd = np.zeros(f.shape), np.zeros(f.shape)
        for c in range(2):
            wv, wb = remap_yardstick(other[..., c], f, method)
            mean = (f[..., c].astype(np.float64) - wv) / 2
            nan = np.isnan(wv)
            out[..., c] = np.where(nan, f[..., c], mean)
            bnd[..., c] = np.where(nan, 0.0, wb / 2 + U * np.abs(np.where(nan, 0.0, mean)))
        return out, bnd
    return half(fwd, bwd), half(bwd, fwd)


# ---- references, computed once and shared by the tests that need them -------------------------------------------------------
@functools.lru_cache(maxsize=None)
def expansion_reference(shape, content, n, sigma):
    """(uint8 frame, its exact blur as float32, value, bound)"""
    img = frame(shape, content)
    blur = blur3_yardstick(img)
    b32 = blur.astype(np.float32)
    assert np.array_equal(b32, blur)                                            # multiples of 1/16: the cast is exact
    value, bound = expansion_yardstick(b32, n, sigma)
    for a in (img, b32, value, bound):
        a.setflags(write=False)
    return img, b32, value, bound


@functools.lru_cache(maxsize=None)
def remap_reference(shape, kind, method):
    """(image, flow, value, bound)"""
    img, flow = remap_image(shape), remap_flow(shape, kind)
    value, bound = remap_yardstick(img, flow, method)
    for a in (img, flow, value, bound):
        a.setflags(write=False)
    return img, flow, value, bound


SMOOTH_SHAPES = ((3, 9), (37, 53), (9, 130))


@functools.lru_cache(maxsize=None)
def smooth_reference(shape, method):
    """(fwd, bwd, (f', bound), (b', bound)): flows of a few pixels, some of them out of the image"""
    fwd, bwd = remap_flow(shape, "amp6", 1), remap_flow(shape, "amp6", 2)
    f, b = smooth_step_yardstick(fwd, bwd, method)
    return fwd, bwd, f, b


def expansion_cases():
    return [(n, sigma, content, shape) for n, sigma in (DEFAULT_POLY, OTHER_POLY) for content in EXPANSION_CONTENTS
            for shape in EXPANSION_SHAPES]


def remap_cases():
    return [(method, shape, kind) for method in REMAP_METHODS for shape in REMAP_SHAPES for kind in REMAP_FLOWS]


def varref_frames(shape, identity):
    """(I0, I1, flow) of the two exact identities: "identical" = one textured frame twice and a zero flow; "constant" = two flat
    frames of different greys and a constant sub-pixel flow"""
    h, w = shape
    if identity == "identical":
        img = frame(shape, "noise", 3) if h * w > 1 else np.full(shape, 200, np.uint8)
        return img, img.copy(), np.zeros(shape + (2,), np.float32)
    flow = np.empty(shape + (2,), np.float32)
    flow[...] = np.array(VARREF_CONSTANT_FLOW, np.float32)
    return np.full(shape, 37, np.uint8), np.full(shape, 201, np.uint8), flow


# ---- judging --------------------------------------------------------------------------------------------------------------
def rejects(got, value, bound):
    """True if `value` (a deliberately wrong statement) is refused by `got` under `bound`: NaN in other places, or a finite
    entry further away than the bound"""
    got, value = np.asarray(got, np.float64), np.asarray(value, np.float64)
    if not np.array_equal(np.isnan(got), np.isnan(value)):
        return True
    ok = ~np.isnan(value)
    return bool((np.abs(got - value)[ok] > np.broadcast_to(bound, value.shape)[ok]).any())


def worst_ratio(got, value, bound):
    """max |got - value| / bound over the finite entries; NaN placement must agree exactly (asserted).  A zero bound demands
    equality (ratio 0 or inf)."""
    got, value = np.asarray(got, np.float64), np.asarray(value, np.float64)
    assert got.shape == value.shape, (got.shape, value.shape)
    nan = np.isnan(value)
    assert np.array_equal(np.isnan(got), nan), f"NaN placement differs at {int((np.isnan(got) != nan).sum())} places"
    if nan.all():
        return 0.0
    err = np.abs(got - value)[~nan]
    b = np.broadcast_to(bound, value.shape)[~nan]
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / b)
    return float(ratio.max())
