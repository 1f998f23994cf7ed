"""The named cases and the parameter table of the navigation-field tests (tests/test_nav_field_contract.py judges them with the two
restatements, tests/test_gpu_nav_field.py runs them on the device, tests/test_nav_field_host.py hands the table to the host's checks).

A case is a box of cells given as occ[z, y, x] (True = occupied), the build's parameters, the goals as cells of the box, and where the
box lies in the shared world: world() is a 256^3 region of unoccupied texels (byte 1, word 0) into which every case's box is written
at its own `lo`, none touching another, so that one upload serves all of them.  `expect` lists (cell, "reached" / "unreached" / a
distance) claims that the contract test holds the restatement to: the case does what its name says."""
import numpy as np

from tests import nav_field_ref as ref

R = 256
G = 8   # the device's levels per launch: the cases that name it are built round this value


def ground(ext, heights):
    """occ of a box of extent (ex, ey, ez): column (x, y) is occupied below heights[y, x]."""
    ex, ey, ez = ext
    h = np.broadcast_to(np.asarray(heights), (ey, ex))
    return np.arange(ez)[:, None, None] < h[None, :, :]


def _case(occ, goals, expect=(), lo=None, **p):
    return dict(occ=np.ascontiguousarray(occ, dtype=bool), goals=[tuple(g) for g in goals], expect=list(expect), lo=lo, p=p)


def _serpentine():
    """Corridors along x at even y, walls three high at odd y with a gap at alternating ends: 40 x 21, the way from (0, 0) to the
    last corridor crosses the tile borders x = 16 and x = 32 in every corridor and is 11 * 39 + 20 = 449 moves long."""
    ex, ey, ez = 40, 21, 5
    occ = ground((ex, ey, ez), 1)
    for y in range(1, ey, 2):
        occ[1:4, y, :] = True
        gap = ex - 1 if (y // 2) % 2 == 0 else 0
        occ[1:4, y, gap] = False
    return occ


def _stairs(rise):
    """Five steps of `rise` along x, two cells deep each; the goal is on the top step."""
    ex, ey, ez = 10, 3, 14
    return ground((ex, ey, ez), 1 + rise * (np.arange(ex) // 2)[None, :])


def _cliff(drop):
    ex, ey, ez = 8, 3, 14
    return ground((ex, ey, ez), np.where(np.arange(ex) < 4, 1 + drop, 1)[None, :])


def _ceiling(with_ceiling):
    """A corridor along x with one step up at x = 5 and, over x = 3..4, a slab two cells above the floor."""
    occ = ground((10, 1, 8), np.where(np.arange(10) < 5, 1, 2)[None, :])
    if with_ceiling:
        occ[3, 0, 3:5] = True
    return occ


def _tunnel():
    occ = ground((9, 1, 5), 1)
    occ[2, 0, 3:6] = True   # free only at z = 1 under it
    return occ


def _ramp():
    """20 x 20 x 256: a ramp that snakes along y, column after column of x, and climbs 0.6 per cell to z = 243."""
    x, y = np.meshgrid(np.arange(20), np.arange(20))
    s = x * 20 + np.where(x % 2 == 0, y, 19 - y)
    return ground((20, 20, 256), 4 + (s * 6) // 10)


def _plate():
    return ground((12, 12, 10), 2)


def cases():
    c = {}
    c["two tiles wide"] = _case(ground((17, 9, 6), 2), [(0, 4, 2)], [((16, 4, 2), 16), ((16, 0, 2), 20), ((3, 3, 3), "unreached")], max_dist=64)
    c["serpentine maze re-enters tiles"] = _case(_serpentine(), [(0, 0, 1)], [((39, 0, 1), 39), ((39, 20, 1), 449), ((0, 1, 4), "unreached")],
                                                 max_dist=4096, max_drop=0)
    c["max_dist a multiple of G"] = _case(ground((30, 1, 3), 1), [(0, 0, 1)], [((2 * G, 0, 1), 2 * G), ((2 * G + 1, 0, 1), "unreached")],
                                          max_dist=2 * G, truncated=1)
    c["max_dist no multiple of G"] = _case(ground((30, 1, 3), 1), [(0, 0, 1)], [((13, 0, 1), 13), ((14, 0, 1), "unreached")], max_dist=13,
                                           truncated=1)
    c["max_dist is the farthest cell"] = _case(ground((30, 1, 3), 1), [(0, 0, 1)], [((29, 0, 1), 29)], max_dist=29, truncated=0)
    for rise in (1, 2):
        for climb in (0, 1, 2):
            top, bottom = (9, 1, 1 + 4 * rise), (0, 1, 1)
            c["stairs of rise %d under max_climb %d" % (rise, climb)] = _case(
                _stairs(rise), [top], [(bottom, 9 if climb >= rise else "unreached"), ((8, 1, 1 + 4 * rise), 1)], max_dist=64, max_climb=climb, max_drop=0)
    for drop, allowed in ((3, 3), (3, 8), (9, 8), (9, 3)):
        c["cliff of %d under max_drop %d" % (drop, allowed)] = _case(
            _cliff(drop), [(7, 1, 1)], [((0, 1, 1 + drop), 7 if allowed >= drop else "unreached"), ((4, 1, 1), 3)], max_dist=64, max_drop=allowed)
    c["the cliff is one-way"] = _case(_cliff(3), [(0, 1, 4)], [((3, 1, 4), 3), ((4, 1, 1), "unreached"), ((7, 1, 1), "unreached")], max_dist=64,
                                      max_drop=3, max_climb=1)
    c["a ceiling forbids the step up but not the walk under it"] = _case(
        _ceiling(True), [(0, 0, 1)], [((4, 0, 1), 4), ((5, 0, 2), "unreached")], max_dist=64, max_climb=1, max_drop=1)
    c["without the ceiling the step is taken"] = _case(_ceiling(False), [(0, 0, 1)], [((4, 0, 1), 4), ((5, 0, 2), 5), ((9, 0, 2), 9)], max_dist=64,
                                                       max_climb=1, max_drop=1)
    c["a tunnel one cell high under height 1"] = _case(_tunnel(), [(0, 0, 1)], [((4, 0, 1), 4), ((8, 0, 1), 8)], max_dist=64, height=1, max_climb=0)
    c["a tunnel one cell high under height 2"] = _case(_tunnel(), [(0, 0, 1)], [((2, 0, 1), 2), ((4, 0, 1), "unreached"), ((8, 0, 1), "unreached")],
                                                       max_dist=64, height=2, max_climb=0)
    c["height 4 at the box's top layer"] = _case(ground((5, 5, 4), 3), [(2, 2, 3)], [((0, 0, 3), 4), ((4, 4, 3), 4)], max_dist=64, height=4)
    c["the bottom layer stands on the floor under the box"] = _case(np.zeros((3, 5, 5), bool), [(0, 0, 0)], [((4, 4, 0), 8), ((2, 2, 1), "unreached")],
                                                                 max_dist=64)
    c["extent 1 in x"] = _case(ground((1, 7, 4), 1), [(0, 0, 1)], [((0, 6, 1), 6)], max_dist=64)
    c["extent 1 in y"] = _case(ground((7, 1, 4), 1), [(6, 0, 1)], [((0, 0, 1), 6)], max_dist=64)
    c["extent 1 in z"] = _case(np.zeros((1, 7, 7), bool), [(3, 3, 0)], [((0, 0, 0), 6), ((6, 6, 0), 6)], max_dist=64, height=4)
    c["the region's far corner"] = _case(ground((19, 18, 5), 2), [(18, 17, 2)], [((0, 0, 2), 35)], lo=(R - 19, R - 18, R - 5), max_dist=64)
    c["several goals"] = _case(_plate(), [(0, 0, 2), (11, 11, 2)], [((5, 5, 2), 10), ((11, 0, 2), 11), ((6, 6, 2), 10)], max_dist=64, used=2, dropped=0)
    # a duplicate, one floating three above the plate (snapped), one six above (too far for goal_snap 4), one outside the box, one
    # inside the ground (candidates go down only)
    c["goals duplicated, snapped and dropped"] = _case(
        _plate(), [(0, 0, 2), (0, 0, 2), (11, 0, 5), (5, 5, 8), (12, 3, 2), (3, 3, 1), (4, -1, 2)], [((0, 0, 2), 0), ((11, 0, 2), 0), ((5, 5, 2), 10)],
        max_dist=64, goal_snap=4, used=3, dropped=4)
    c["no goal"] = _case(_plate(), [], [((0, 0, 2), "unreached")], max_dist=64, used=0, dropped=0)
    return c


def big_cases():
    """The cases above 48 x 48 x 24 that need no world of their own."""
    return {"z extent 256 on a 20 x 20 footprint": _case(_ramp(), [(19, 0, 243)], [((0, 0, 4), "reached"), ((0, 0, 5), "unreached")], max_dist=1024, max_climb=1, max_drop=1)}


def placed(all_cases):
    """Gives every case without a `lo` one in the shared world: slots of 48 x 48 x 32 from (1, 3, 5) on (odd, so no box is aligned to a
    brick), the big ones after them.  Returns the cases."""
    slot = 0
    for name, c in all_cases.items():
        if c["lo"] is not None:
            continue
        ez, ey, ex = c["occ"].shape
        if ez <= 32:
            c["lo"] = (1 + 49 * (slot % 4), 3 + 49 * ((slot // 4) % 4), 5 + 33 * (slot // 16))
            slot += 1
        else:
            c["lo"] = (200, 205, 0)
    return all_cases


def params_of(c):
    p = {k: v for k, v in c["p"].items() if k in ("max_dist", "height", "max_climb", "max_drop", "goal_snap")}
    return ref.params(c["lo"], **p)


def goals_of(c):
    """The case's goals as texels, int[N, 3]."""
    return np.asarray(c["goals"], dtype=np.int64).reshape(-1, 3) + np.asarray(c["lo"], dtype=np.int64)


def ext_of(c):
    return c["occ"].shape[::-1]


def world(all_cases):
    """(mats u32, mine u8) [z, y, x] of the shared region with every placed case's box written into it."""
    mine = np.ones((R, R, R), dtype=np.uint8)
    mats = np.zeros((R, R, R), dtype=np.uint32)
    taken = np.zeros((R, R, R), dtype=bool)
    for name, c in all_cases.items():
        lo, (ex, ey, ez) = c["lo"], ext_of(c)
        sl = (slice(lo[2], lo[2] + ez), slice(lo[1], lo[1] + ey), slice(lo[0], lo[0] + ex))
        assert not taken[sl].any(), name
        taken[sl] = True
        mine[sl] = np.where(c["occ"], 0, 1)
        mats[sl] = np.where(c["occ"], 0x00808080, 0)
    return mats, mine


def every_cell_agents(lo, ext, snap_down=0, snap_up=0):
    """One agent at the centre of every cell of the box, x fastest."""
    z, y, x = np.meshgrid(np.arange(ext[2]), np.arange(ext[1]), np.arange(ext[0]), indexing="ij")
    a = np.zeros(x.size, dtype=ref.AGENT_DTYPE)
    a["pos"] = np.stack([x.ravel() + lo[0] + 0.5, y.ravel() + lo[1] + 0.5, z.ravel() + lo[2] + 0.25], axis=1)
    a["snap_down"], a["snap_up"] = snap_down, snap_up
    return a


def odd_agents(lo, ext):
    """Agents that try the sample's edges on a field over [lo, lo + ext): positions exactly on integer z, just outside the box on
    every side, snaps at their limits and beyond, NaN, +-inf, +-2^20 and just below, a non-zero reserved byte."""
    rows = []

    def add(pos, down=1, up=1, res=(0, 0)):
        rows.append((tuple(float(v) for v in pos), down, up, res))
    cx, cy = lo[0] + ext[0] // 2 + 0.5, lo[1] + ext[1] // 2 + 0.5
    for z in range(lo[2] - 3, lo[2] + ext[2] + 3):
        for down, up in ((0, 0), (8, 2), (8, 0), (0, 2), (1, 1)):
            add((cx, cy, z), down, up)
            add((cx, cy, z + 0.999), down, up)
    for dx, dy in ((-0.001, 0), (ext[0], 0), (0, -0.001), (0, ext[1])):
        add((lo[0] + dx + (0.5 if dy else 0), lo[1] + dy + (0.5 if dx else 0), lo[2] + 2.5), 8, 2)
    add((lo[0] + 0.5, lo[1] + 0.5, lo[2] + 2.5), 9, 0)
    add((lo[0] + 0.5, lo[1] + 0.5, lo[2] + 2.5), 0, 3)
    add((lo[0] + 0.5, lo[1] + 0.5, lo[2] + 2.5), 1, 1, (1, 0))
    add((lo[0] + 0.5, lo[1] + 0.5, lo[2] + 2.5), 1, 1, (0, 255))
    for bad in (np.nan, np.inf, -np.inf, 2.0 ** 20, -2.0 ** 20):
        for k in range(3):
            pos = [lo[0] + 0.5, lo[1] + 0.5, lo[2] + 2.5]
            pos[k] = bad
            add(pos)
    add((2.0 ** 20 - 0.0625, -(2.0 ** 20) + 0.0625, lo[2] + 2.5))
    a = np.zeros(len(rows), dtype=ref.AGENT_DTYPE)
    for i, r in enumerate(rows):
        a[i] = r
    return a


# ---- the parameter table of the host's checks: (max_dist, height, max_climb, max_drop, goal_snap, reserved, goal_count, goals_null) ---
def build_table():
    ok = (64, 2, 1, 3, 0, (0, 0, 0), 1, 0)
    rows = [ok]
    for i, values in enumerate(((0, 1, 4096, 4097, 0xFFFFFFFF), (0, 1, 4, 5, 255), (0, 2, 3, 255), (0, 8, 9, 255), (0, 8, 9, 255))):
        for v in values:
            rows.append(ok[:i] + (v,) + ok[i + 1:])
    rows += [ok[:5] + (r,) + ok[6:] for r in ((1, 0, 0), (0, 1, 0), (0, 0, 0x80000000))]
    rows += [ok[:6] + t for t in ((0, 0), (0, 1), (1, 1), (4096, 0), (4097, 0), (4097, 1))]
    return rows


def box_table():
    """(lo, ext, logr) rows of the box test."""
    return [((0, 0, 0), (256, 256, 256), 8), ((1, 0, 0), (256, 256, 256), 8), ((0, 0, 1), (1, 1, 255), 8), ((0, 0, 1), (1, 1, 256), 8),
            ((-1, 0, 0), (4, 4, 4), 8), ((255, 255, 255), (1, 1, 1), 8), ((256, 0, 0), (1, 1, 1), 8), ((300, 300, 300), (200, 212, 212), 9),
            ((300, 300, 300), (200, 213, 212), 9), ((1000, 1000, 1000), (24, 24, 24), 10), ((0x7FFFFFFF, 0, 0), (256, 1, 1), 10)]


def plan_table():
    """(ext, max_dist, levels) rows of the plan: the largest field and others."""
    return [((256, 256, 256), 4096, 8), ((256, 256, 256), 4096, 1), ((17, 9, 6), 64, 8), ((1, 1, 1), 1, 8), ((16, 16, 1), 7, 8), ((16, 16, 1), 8, 8),
            ((33, 47, 200), 15, 4), ((96, 96, 64), 64, 4), ((192, 192, 128), 384, 8), ((255, 31, 2), 4095, 1)]
