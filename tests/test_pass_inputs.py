"""The inputs of tests/test_gpu_pass_worlds.py, checked on the CPU with the restatements alone (tests/point_light_ref.py,
light_shadow_ref.py, entity_shadow_ref.py) on frames drawn by the oracle: the worlds and poses of tests/pass_worlds.py do reach the
branches that terrain cannot — shadow rays that start on a 0 texel, minefield values above 6 and above 15 under a surface point,
sun rays and shadow rays that end at RT_TRACE_LIMIT, pixels an entity shades with and without the world — and a restatement with one
of these rules wrong gives other planes on these very inputs, so that the kernels' agreement there means something.

Every floor is a condition on the inputs, not on the library."""
import contextlib

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import entity_shadow_ref as es
from tests import light_shadow_ref as ls
from tests import pass_worlds as pw
from tests import point_light_ref as pl

pytestmark = pytest.mark.usefixtures("native_built")

SID = 1                                   # the id the first rt_stamp_create of a context returns
WRONG_RULES = ["capped at 6", "masked to 4 bits", "limit leaves", "fresh on 0 is open"]


class Inputs:
    """One frame of a world (spp 1, depth 2, by the oracle) with the records the GPU tests scatter on it."""

    def __init__(self, name, R, pose, noise, shape=pw.SHAPES[0], nlights=16):
        self.name, self.R, (self.W, self.H) = name, R, shape
        W, H = shape
        self.mats, self.mine = pw.world_of(name, R)
        self.u = pw.uniforms(po, name, R, pose)
        self.planes, _ = po.render(self.mats, self.mine, noise, self.u, W, H, 1, 2, region=R)
        self.stamps = {SID: es.small_stamp()}
        seed = 3
        self.lights = pw.scatter_lights(self.planes, self.u, W, H, nlights, seed, rmin=4.0, rmax=200.0 if name == "limit" else 40.0)
        self.boxes, self.models = pw.occluders(self.planes, self.u, W, H, self.lights, 30, 10, seed, SID)
        self.sun_boxes = pw.sun_boxes(self.planes, self.u, W, H, 40, seed)
        self.sun_models = es.scatter_models(self.planes, self.u, W, H, 12, seed, SID, pw.STAMP_EXTENT, scales=(1.0, 0.125))

    def lit(self):
        return pl.add_lights(self.planes, self.u, self.lights, self.mine, self.W, self.H, self.R)

    def occluded(self, classes=None):
        return ls.add_lights_occluded(self.planes, self.u, self.lights, self.boxes, self.models, self.stamps, self.mine, self.W, self.H, self.R,
                                      classes=classes)

    def masks(self):
        return es.masks(self.planes, self.u, self.sun_boxes, self.sun_models, self.stamps, self.mine, self.W, self.H, self.R)

    def shaded(self):
        return es.shadow_entities(self.planes, self.u, self.sun_boxes, self.sun_models, self.stamps, self.mine, self.W, self.H, self.R, 0.75)

    def light_classes(self):
        classes = {}
        self.occluded(classes)
        return classes

    def pairs(self, lights=None):
        return pw.light_pairs(self.planes, self.u, self.lights if lights is None else lights, self.mine, self.W, self.H, self.R)

    def sun_kinds(self):
        return pw.sun_kinds(self.planes, self.u, self.mine, self.W, self.H, self.R)[1]

    def under(self):
        """The minefield value under the P' of every surface pixel."""
        surface, P, _, _ = pl.surface_points(self.planes, self.u, self.W, self.H)
        return pw.fetch_under(self.mine, self.R, P[surface])


_MADE = {}


@pytest.fixture
def inputs(blue_noise):
    def get(name, R, pose, shape=pw.SHAPES[0], nlights=16):
        key = (name, R, int(pose), shape, nlights)
        if key not in _MADE:
            for k in [k for k in _MADE if k[:2] != (name, R) and k[1] > 256]:
                del _MADE[k]
            _MADE[key] = Inputs(name, R, pose, blue_noise, shape, nlights)
        return _MADE[key]
    return get


def differing(a, b):
    """In how many pixels two sets of planes differ."""
    bad = False
    for name in a:
        h, w = a[name].shape[:2]
        bad = bad | (a[name].reshape(h, w, -1).view(np.uint8) != b[name].reshape(h, w, -1).view(np.uint8)).any(axis=-1)
    return int(np.sum(bad))


# ---- the floors ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [256, 512])
def test_arbitrary_world_reaches_the_branches(R, inputs):
    both = [inputs("arbitrary", R, pose) for pose in (pw.PLAIN, pw.SCROLLED)]
    for f in both:
        pairs = f.pairs()
        assert pairs["visible"] >= 200 and pairs["blocked"] >= 100, pairs
        assert int((f.sun_kinds() == es.AIR).sum()) >= 50
    under = np.concatenate([f.under() for f in both])
    assert int((under == 0).sum()) >= 1            # a fresh shadow ray and a fresh sun ray on a 0 texel
    assert int(under.max()) >= 15                   # a first step longer than any palette value gives, past the nibble map's 15


def test_the_on_zero_pose_starts_shadow_rays_on_0_texels(inputs):
    f = inputs("arbitrary", 256, pw.ON_ZERO)
    under, pairs = f.under(), f.pairs()
    assert int((under == 0).sum()) >= 50 and int((under != 0).sum()) >= 50 and int(under.max()) >= 15
    assert pairs["visible"] >= 200 and pairs["blocked"] >= 100, pairs


def test_pyramid_world_reaches_the_branches(inputs):
    for scrolled in (False, True):
        f = inputs("pyramid", 256, scrolled)
        pairs = f.pairs()
        assert pairs["visible"] >= 200 and pairs["blocked"] >= 200, pairs
    assert int(f.under().max()) >= 7                # (the scrolled pose)


def test_limit_window_reaches_the_trace_limit(inputs):
    for pose in (pw.PLAIN, pw.SCROLLED):
        f = inputs("limit", 256, pose)
        kinds, masks = f.sun_kinds(), f.masks()
        assert int((kinds == es.LIMIT).sum()) >= 50
        # ... and under an entity: where rt_shadow_entities must find no sun term to remove
        assert int(((masks["changed"] | masks["world"]) & (kinds == es.LIMIT)).sum()) >= 50
    f = inputs("limit", 256, pw.PLAIN)               # (a stalled shadow ray costs the restatement 2048 steps: one pose)
    assert f.pairs()["limit"] >= 20                  # the scattered lights (radii up to 200) ...
    along = pw.limit_lights(f.planes, f.u, f.W, f.H, 3, 5)
    assert f.pairs(along)["limit"] >= 20             # ... and lights of radius 1024 along the stall direction


@pytest.mark.parametrize("name,R,pose", [("arbitrary", 256, 0), ("arbitrary", 256, 1), ("arbitrary", 512, 0), ("arbitrary", 512, 1), ("pyramid", 256, 1),
                                         ("limit", 256, 0)])
def test_occluders_shade_with_and_without_the_world(name, R, pose, inputs):
    f = inputs(name, R, pose)
    masks = f.masks()
    assert int(masks["changed"].sum()) >= 30 and int(masks["world"].sum()) >= 30, {k: int(v.sum()) for k, v in masks.items()}
    classes = f.light_classes()
    assert classes["entity_only"] >= 30 and classes["both"] >= 30, classes


def test_the_probe_restatement_agrees_with_itself_through_either_trace(inputs, blue_noise):
    """tests/light_probe_ref.py through tests/ray_query_ref.py (what the GPU test uses above region 256) against the same through the
    oracle's trace_ray, on the arbitrary world."""
    from tests import light_probe_ref as lp
    f = inputs("arbitrary", 256, pw.PLAIN)
    p = pw.poses("arbitrary")[pw.PLAIN]
    rng = np.random.default_rng(1)
    trace = lp.restated_trace(f.mats, f.mine, p["lr"], 256)
    for k in range(8):
        pos = (np.array(p["origin"]) + rng.uniform(-20, 20, 3)).astype(np.float32)
        a = lp.probe_light(f.mats, f.mine, blue_noise, p["sun"], 7, p["lr"], pos, k % 7, (k, 2 * k), 4, 3)
        b = lp.probe_light(f.mats, f.mine, blue_noise, p["sun"], 7, p["lr"], pos, k % 7, (k, 2 * k), 4, 3, trace=trace)
        assert a[0].view(np.uint32).tolist() == b[0].view(np.uint32).tolist() and a[1] == b[1], (k, a, b)


# ---- sensitivity: a restatement with one rule wrong gives other planes on these inputs ---------------------------------------------------------
@contextlib.contextmanager
def wrong_rule(rule):
    """tests/point_light_ref and tests/entity_shadow_ref with one rule of the walk wrong, through their `_fetch` or round their
    trace functions; the restatements themselves are not forked."""
    saved = [(m, n, getattr(m, n)) for m, n in ((pl, "_fetch"), (es, "_fetch"), (pl, "trace_visible"), (es, "trace_kind"))]
    fetch_pl, fetch_es, visible, kind = (s[2] for s in saved)
    try:
        if rule in ("capped at 6", "masked to 4 bits"):
            wrong = (lambda v: np.minimum(v, 6)) if rule == "capped at 6" else (lambda v: v & 15)
            pl._fetch = lambda mine, R, pos: wrong(fetch_pl(mine, R, pos))
            es._fetch = lambda mine, R, pos: wrong(fetch_es(mine, R, pos))
        elif rule == "limit leaves":
            def trace_visible(minefield, region, lr, origin, v, dist2, ends=False):
                vis, end = visible(minefield, region, lr, origin, v, dist2, ends=True)
                vis = vis | (end == pl.END_LIMIT)
                return (vis, end) if ends else vis

            def trace_kind(minefield, region, lr, origin, direction):
                k = kind(minefield, region, lr, origin, direction)
                return np.where(k == es.LIMIT, es.AIR, k)
            pl.trace_visible, es.trace_kind = trace_visible, trace_kind
        elif rule == "fresh on 0 is open":
            fresh = [False]                          # the next fetch is a ray's first

            def first_is_open(fetch):
                def f(mine, R, pos):
                    v = fetch(mine, R, pos)
                    if fresh[0]:
                        fresh[0] = False
                        v = np.where(v == 0, 1, v)
                    return v
                return f

            def arm(trace):
                def f(*a, **kw):
                    fresh[0] = True
                    try:
                        return trace(*a, **kw)
                    finally:
                        fresh[0] = False
                return f
            pl._fetch, es._fetch = first_is_open(fetch_pl), first_is_open(fetch_es)
            pl.trace_visible, es.trace_kind = arm(visible), arm(kind)
        else:
            raise ValueError(rule)
        yield
    finally:
        for m, n, v in saved:
            setattr(m, n, v)


# (wrong rule, world, region, pose, pass, lights): the pairs in which the rule can be seen in more than 10 pixels of a 52 x 36 frame.
# The others cannot reach that on these inputs and are left out: every rule on the pyramid world (a legal distance bound gives the
# same verdicts capped, holds no value above 9, no stall and no P' on a 0 texel), the two value rules in the limit window (terrain:
# values 0..6) and the limit rule outside it, "fresh on 0 is open" on every pose but ON_ZERO (at most 10 surface points lie on a 0
# texel) and for the sun everywhere (round such a point the sun ray is blocked one step later anyway).
PLAIN, SCROLLED, ON_ZERO = pw.PLAIN, pw.SCROLLED, pw.ON_ZERO
SENSITIVE = [
    ("capped at 6", "arbitrary", 256, PLAIN, "lights", 70), ("capped at 6", "arbitrary", 256, PLAIN, "sun", 16),
    ("capped at 6", "arbitrary", 256, SCROLLED, "sun", 16), ("capped at 6", "arbitrary", 256, ON_ZERO, "lights", 16),
    ("capped at 6", "arbitrary", 512, PLAIN, "sun", 16), ("capped at 6", "arbitrary", 512, SCROLLED, "lights", 70),
    ("capped at 6", "arbitrary", 512, SCROLLED, "sun", 16),
    ("masked to 4 bits", "arbitrary", 256, PLAIN, "lights", 70), ("masked to 4 bits", "arbitrary", 256, SCROLLED, "lights", 70),
    ("masked to 4 bits", "arbitrary", 256, SCROLLED, "sun", 16), ("masked to 4 bits", "arbitrary", 256, ON_ZERO, "lights", 16),
    ("masked to 4 bits", "arbitrary", 512, SCROLLED, "lights", 70), ("masked to 4 bits", "arbitrary", 512, SCROLLED, "sun", 16),
    ("limit leaves", "limit", 256, PLAIN, "lights", 16), ("limit leaves", "limit", 256, PLAIN, "sun", 16),
    ("limit leaves", "limit", 256, SCROLLED, "sun", 16),
    ("fresh on 0 is open", "arbitrary", 256, ON_ZERO, "lights", 16),
]


@pytest.mark.parametrize("rule,name,R,pose,which,nlights", SENSITIVE,
                         ids=["%s-%s%d-pose%d-%s" % (r.replace(" ", "_"), n, R, p, w) for r, n, R, p, w, _ in SENSITIVE])
def test_a_wrong_rule_shows_on_these_inputs(rule, name, R, pose, which, nlights, inputs):
    f = inputs(name, R, pose, nlights=nlights)
    run = f.lit if which == "lights" else f.shaded
    true = run()
    with wrong_rule(rule):
        wrong = run()
    assert differing(true, run()) == 0              # (the patch is gone)
    n = differing(true, wrong)
    print("%s on %s %d pose %d, %s: %d pixels differ" % (rule, name, R, pose, which, n))
    assert n > 10
