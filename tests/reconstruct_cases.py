"""Shared cases of the reconstruction tests, and an evaluation of the definitions of utils/reconstruct.py that is written differently from
the product's host form (directional sweeps over ordered integer keys) and from the kernels (tile sweeps over the same keys): THE TEXTBOOK
ITERATION on float64 values -- ``R <- minimum(scipy.ndimage.grey_dilation(R, footprint, mode="constant", cval=-inf), mask)`` until nothing
changes, no heap, no keys --, the regional maxima by LABELLING THE PLATEAUS of every distinct value with ``scipy.ndimage.label`` and
testing each plateau's dilated maximum, the h-maxima as the composition of the two, and ``scipy.ndimage.binary_fill_holes`` for masks.
Erosion and the minima are the model of the negated image.  Positions outside the domain hold ``-inf`` in the model's mask and in its
``R``, so they offer nothing to a neighbour.

Every case stays near 20 k positions so that the model takes about a second; expectations are computed once per session."""
import functools

import numpy as np
from scipy import ndimage

import watershed_cases as WC

CONNECTIVITIES = {2: (4, 8), 3: (6, 26)}
TOP = {np.dtype(np.float32): np.inf, np.dtype(np.float16): np.inf, np.dtype(np.uint8): 255, np.dtype(np.int16): 32767, np.dtype(bool): 1}


# ---------------------------------------------------------------------------------------------------------------- the model
def footprint(dims, full):
    return ndimage.generate_binary_structure(dims, dims if full else 1)


def iterate(start, mask, fp):
    """the least fixed point above ``min(start, mask)`` of one entry, float64; ``-inf`` marks the outside of the domain in ``mask``"""
    r = np.minimum(start, mask)
    while True:
        nxt = np.minimum(ndimage.grey_dilation(r, footprint=fp, mode="constant", cval=-np.inf), mask)
        if np.array_equal(nxt, r):
            return r
        r = nxt


def plateau_maxima(v, inside, fp):
    """the regional maxima of one entry: the plateaus (connected sets of one value inside the domain) whose dilation sees nothing higher"""
    low = np.where(inside, v, -np.inf)
    around = ndimage.grey_dilation(low, footprint=fp, mode="constant", cval=-np.inf)
    out = np.zeros(v.shape, bool)
    for value in np.unique(v[inside]):
        lab, n = ndimage.label(inside & (v == value), structure=fp)
        if n:
            highest = ndimage.maximum(around, lab, np.arange(1, n + 1))
            out |= np.concatenate([[False], highest <= value])[lab]
    return out


class Case:
    """``op``: "reconstruction" | "regional" | "h" | "fill"; ``image`` (the mask of a reconstruction), ``seed`` (reconstruction only), ``domain`` (bool or None),
    ``h``; ``mirror``: erosion / the minima"""

    def __init__(self, name, op, image, seed=None, domain=None, h=None, mirror=False, dims=2, connectivities=None):
        assert domain is None or domain.shape == image.shape
        self.name, self.op, self.image, self.seed, self.domain, self.h, self.mirror, self.dims = name, op, image, seed, domain, h, mirror, dims
        self.connectivities = connectivities or CONNECTIVITIES[dims]

    def __repr__(self):
        return self.name

    def entries(self, a):
        return a.reshape((-1,) + a.shape[a.ndim - self.dims:])

    @functools.cached_property
    def inside(self):
        ok = ~np.isnan(self.image.astype(np.float64))
        return ok if self.domain is None else ok & (self.domain != 0)

    @functools.lru_cache(maxsize=None)
    def expected(self, connectivity):
        """the result of the definition as an array of the result's dtype; value comparisons are made on the bits"""
        fp = footprint(self.dims, connectivity == CONNECTIVITIES[self.dims][1])
        sign = -1.0 if self.mirror or self.op == "fill" else 1.0                                   # (hole filling is an erosion)
        img32 = self.image.astype(np.float32)
        v = sign * (np.where(self.inside, img32, 0).astype(np.float64) + 0.0)                      # (-0.0 + 0.0 is +0.0)
        out = np.empty(self.image.shape, bool if self.op in ("regional", "h") else self.image.dtype)
        if self.op == "reconstruction":
            s = self.seed.astype(np.float64)
            s = sign * (np.where(np.isnan(s), -sign * np.inf, s) + 0.0)                            # a NaN seed: the lowest value (mirror: the highest)
        elif self.op == "h":
            with np.errstate(invalid="ignore"):
                cut = img32 + np.float32(self.h) if self.mirror else img32 - np.float32(self.h)     # ONE float32 operation, as the product does
            s = sign * (np.where(self.inside, cut, 0).astype(np.float64) + 0.0)
        else:
            s = None
        for k, (ve, ie, oe) in enumerate(zip(self.entries(v), self.entries(self.inside), self.entries(out))):
            m = np.where(ie, ve, -np.inf)
            if self.op == "regional":
                oe[...] = plateau_maxima(ve, ie, fp)
                continue
            if self.op == "h":
                hmax = iterate(np.where(ie, self.entries(s)[k], -np.inf), m, fp)
                oe[...] = plateau_maxima(hmax, ie, fp)
                continue
            if self.op == "fill":
                border = np.zeros(ve.shape, bool)
                for ax in range(ve.ndim):
                    border[(slice(None),) * ax + (0,)] = border[(slice(None),) * ax + (-1,)] = True
                if self.image.dtype == bool and self.domain is None:
                    oe[...] = ndimage.binary_fill_holes(self.entries(self.image)[k], structure=fp)
                    continue
                start = np.where(border, ve, -np.inf)                                              # (mirrored: +inf off the faces)
                start = np.where(ie, start, -np.inf)
                reached = iterate(np.where(border & ie, np.inf, -np.inf), np.where(ie, np.inf, -np.inf), fp) == np.inf
            else:
                start = np.where(ie, self.entries(s)[k], -np.inf)
                reached = ie
            r = sign * iterate(start, m, fp)
            top = TOP[self.image.dtype]
            r = np.where(reached, r, top)                                                          # fill: what no face reaches holds the dtype's highest value
            with np.errstate(invalid="ignore"):
                oe[...] = np.where(ie, r.astype(self.image.dtype), self.entries(self.image)[k])
        out.setflags(write=False)
        return out


def same_bits(got, want):
    """bit for bit, for every dtype (NaNs outside the domain compare by their bits)"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


# ---------------------------------------------------------------------------------------------------------------- generators
def plateau_noise(shape, seed, sigma=3.0):
    """smoothed noise quantised to steps of 1 / 40: plateaus, and values every float type of the tests holds exactly once scaled by 40"""
    v = WC.smooth_noise(shape, seed, sigma)
    return (np.round(v / v.std() * 8) / 40).astype(np.float32)


def holes_mask(shape, seed, count, radius):
    """blobs with random holes punched into them"""
    rng = np.random.default_rng(seed)
    sem = WC.blob_map(shape, seed, count=count, radius=radius)
    return sem & ~WC.blob_map(shape, seed + 1, count=3 * count, radius=(1, max(2, radius[0] // 3))) | (rng.random(shape) < 0.01)


H_ROW = np.array([[0, 1, 3, 5, 3, 2, 2.5, 3, 2.5, 1, 0]], np.float32)
H_ROW_RESULTS = {0.5: [0, 0, 0, 1, 0, 0, 1, 1, 1, 0, 0], 1.0: [0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0], 1.5: [0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0],
                 3.5: [0, 0, 1, 1, 1, 1, 1, 1, 1, 0, 0]}
SERPENTINE_POSITIONS = 8580                 # the corridor of the sweep-loop case: the value takes one step less


def _cases():
    c = {}

    def add(case):
        assert case.name not in c
        c[case.name] = case

    def family(name, image, seed, dims=2, domain=None):
        """every operation on one image: reconstruction both ways from a lowered / raised copy, the extrema, the h-extrema"""
        rng = np.random.default_rng(seed)
        drop = (rng.random(image.shape) * 0.3).astype(np.float32)
        add(Case(name + "/dilation", "reconstruction", image, seed=(image - drop).astype(image.dtype), domain=domain, dims=dims))
        add(Case(name + "/erosion", "reconstruction", image, seed=(image + drop).astype(image.dtype), domain=domain, mirror=True, dims=dims))
        add(Case(name + "/maxima", "regional", image, domain=domain, dims=dims))
        add(Case(name + "/minima", "regional", image, domain=domain, mirror=True, dims=dims))
        add(Case(name + "/h_maxima", "h", image, domain=domain, h=0.1, dims=dims))
        add(Case(name + "/h_minima", "h", image, domain=domain, h=0.075, mirror=True, dims=dims))

    family("odd_width", plateau_noise((100, 99), 1), seed=1)                                        # rows that start at every alignment
    family("wide", plateau_noise((96, 104), 2), seed=2)                                             # the wide arm
    add(Case("odd_total/h_maxima", "h", plateau_noise((37, 53), 3), h=0.1))                          # 1961 positions, not a multiple of 4: the peeled arm
    add(Case("odd_total/dilation", "reconstruction", plateau_noise((37, 53), 3), seed=plateau_noise((37, 53), 3) - np.float32(0.2)))
    for e in ((63, 65), (64, 64), (65, 129)):                                                       # either side of every tile edge
        img = plateau_noise(e, 10 + e[0] + e[1])
        add(Case("tile%dx%d/h_maxima" % e, "h", img, h=0.1))
        add(Case("tile%dx%d/minima" % e, "regional", img, mirror=True))
        add(Case("tile%dx%d/fill" % e, "fill", img))
    for e in ((7, 9, 33), (8, 8, 32), (9, 17, 65)):                                                 # either side of every brick edge
        img = plateau_noise(e, 20 + e[0] + e[2], 1.5)
        add(Case("brick%dx%dx%d/h_maxima" % e, "h", img, h=0.1, dims=3))
        add(Case("brick%dx%dx%d/maxima" % e, "regional", img, dims=3))
        add(Case("brick%dx%dx%d/erosion" % e, "reconstruction", img, seed=img + np.float32(0.25), mirror=True, dims=3))
        add(Case("brick%dx%dx%d/fill" % e, "fill", img, dims=3))
    sem = WC.blob_map((96, 120), 11)                                                                # the recipe: the distance map inside the blobs
    d = ndimage.distance_transform_edt(sem).astype(np.float32)
    add(Case("blobs/h_maxima", "h", d, domain=sem, h=2.0))
    add(Case("blobs/maxima", "regional", d, domain=sem))
    add(Case("blobs/dilation", "reconstruction", d, seed=d - np.float32(2.0), domain=sem))
    moat = sem.copy()                                                                               # a moat one position inside the left half of the border:
    moat[1, :60] = moat[-2, :60] = moat[:, 1] = False                                               # components of the domain that touch no face
    add(Case("blobs/fill_domain", "fill", plateau_noise((96, 120), 12), domain=moat))
    sem3 = WC.blob_map((17, 24, 40), 74, count=10, radius=(4, 7))
    add(Case("volume_blobs/h_maxima", "h", ndimage.distance_transform_edt(sem3).astype(np.float32), domain=sem3, h=1.0, dims=3))
    for h in H_ROW_RESULTS:
        add(Case(f"row/h{h}", "h", H_ROW, h=h, connectivities=(4,)))
    add(Case("constant/maxima", "regional", np.full((20, 30), 1.5, np.float32)))
    add(Case("constant/h_maxima", "h", np.full((2, 20, 30), -3.0, np.float32), h=1.0))
    img = plateau_noise((50, 60), 30)
    rng = np.random.default_rng(31)
    seed = np.where(rng.random((50, 60)) < 0.2, img + np.float32(0.5), img - np.float32(0.3)).astype(np.float32)
    add(Case("clamp/dilation", "reconstruction", img, seed=seed))                                   # seed > mask in places
    add(Case("clamp/erosion", "reconstruction", img, seed=(2 * img - seed).astype(np.float32), mirror=True))
    odd = plateau_noise((50, 60), 32)
    odd[rng.random((50, 60)) < 0.06] = np.nan
    odd[rng.random((50, 60)) < 0.05] = np.inf
    odd[rng.random((50, 60)) < 0.05] = -np.inf
    odd[rng.random((50, 60)) < 0.1] = -0.0
    odd[rng.random((50, 60)) < 0.1] = 0.0
    assert np.signbit(odd[odd == 0]).any() and np.isnan(odd).any()
    sd = (odd - np.float32(0.2)).astype(np.float32)
    sd[rng.random((50, 60)) < 0.1] = np.nan
    sd[rng.random((50, 60)) < 0.05] = -0.0
    for op, kw in (("dilation", dict(seed=sd)), ("erosion", dict(seed=np.where(np.isnan(sd), sd, odd + np.float32(0.2)).astype(np.float32), mirror=True))):
        add(Case("odd_values/" + op, "reconstruction", odd, **kw))
    add(Case("odd_values/maxima", "regional", odd))
    add(Case("odd_values/minima", "regional", odd, mirror=True))
    add(Case("odd_values/h_maxima", "h", odd, h=0.1))
    add(Case("odd_values/h_minima", "h", odd, h=0.1, mirror=True))
    add(Case("odd_values/fill", "fill", odd))
    family("stack", plateau_noise((3, 40, 50), 40), seed=40)                                        # independent entries
    add(Case("stack/fill", "fill", plateau_noise((3, 40, 50), 40)))
    vs = plateau_noise((2, 9, 10, 35), 41, 1.5)
    add(Case("volume_stack/h_maxima", "h", vs, h=0.1, dims=3))
    add(Case("volume_stack/dilation", "reconstruction", vs, seed=vs - np.float32(0.15), dims=3))
    add(Case("volume_stack/fill", "fill", vs, dims=3))
    for k, shape in enumerate(((90, 110), (3, 40, 50))):                                            # random masks with holes, against scipy
        add(Case("holes%d/fill" % k, "fill", holes_mask(shape, 50 + k, 9, (7, 15))))
    add(Case("holes_u8/fill", "fill", holes_mask((37, 53), 53, 5, (6, 12)).astype(np.uint8)))
    add(Case("holes_volume/fill", "fill", holes_mask((17, 24, 40), 54, 8, (4, 8)), dims=3))
    add(Case("holes_volume_stack/fill", "fill", holes_mask((2, 9, 17, 33), 56, 4, (3, 6)), dims=3))
    add(Case("grey/fill", "fill", plateau_noise((80, 90), 57)))                                     # the grey form
    add(Case("grey_i16/fill", "fill", (plateau_noise((60, 70), 58) * 40).astype(np.int16)))
    # the sweep loop: a constant mask on the long serpentine corridor, one high seed at its start -- the value has to travel the whole
    # corridor, through nine tiles, back and forth
    corridor, markers = WC.serpentine(130, 131)
    assert int(corridor.sum()) == SERPENTINE_POSITIONS
    add(Case("serpentine_long/dilation", "reconstruction", np.full((130, 131), 2.0, np.float32), seed=np.where(markers != 0, 2.0, 0.0).astype(np.float32), domain=corridor,
             connectivities=(4,)))
    return c


CASES = _cases()
assert all(c.image.size <= 21_000 for c in CASES.values()), [n for n, c in CASES.items() if c.image.size > 21_000]
PAIRS = [(n, k) for n, c in CASES.items() for k in c.connectivities]
