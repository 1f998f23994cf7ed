"""The rules of the navigation fields (include/rt_abi.h "Navigation fields"), stated twice in numpy, independently: neither
restatement shares a helper with the other beyond reading the world (box_occupied).

  build_graph / sample_loop : the explicit move graph, cell by cell, and a queue; the sample as a loop over agents.
  build_dilate / sample_array : level-synchronous dilation with whole-array shifts; the sample on whole arrays.

Both take the box's occupancy occ[z, y, x] (bool), the parameters `p` (a dict: lo, max_dist, height, max_climb, max_drop, goal_snap),
the goals as int[N, 3] texels and the result record before the call, and return (dist u16[ez, ey, ex], move u8[ez, ey, ex], result).
The host's verdicts and launch plan (raytrace_amd/csrc/api/nav_check.hpp) are restated at the end."""
import collections

import numpy as np

UNREACHED, NO_MOVE = 0xFFFF, 0xFF
RESULT_DTYPE = np.dtype([("standable", "<u4"), ("reached", "<u4"), ("levels", "<u4"), ("truncated", "<u4"), ("goals_used", "<u4"),
                         ("goals_dropped", "<u4"), ("reserved", "<u4", 2)])
GOAL_DTYPE = np.dtype([("cell", "<i4", 3), ("reserved", "<u4")])
AGENT_DTYPE = np.dtype([("pos", "<f4", 3), ("snap_down", "u1"), ("snap_up", "u1"), ("reserved", "u1", 2)])
STEP_DTYPE = np.dtype([("cell", "<i4", 3), ("dist", "<u4"), ("next", "<i4", 3), ("move", "<u4")])
STEPS_H = ((1, 0), (-1, 0), (0, 1), (0, -1))   # b.xy - a.xy of h = 0..3


def params(lo, max_dist, height=2, max_climb=1, max_drop=3, goal_snap=0):
    return dict(lo=tuple(int(v) for v in lo), max_dist=int(max_dist), height=int(height), max_climb=int(max_climb), max_drop=int(max_drop),
                goal_snap=int(goal_snap))


def result0(standable=0, reached=0, levels=0, truncated=0, goals_used=0, goals_dropped=0, reserved=(0, 0)):
    r = np.zeros(1, dtype=RESULT_DTYPE)
    r[0] = (standable, reached, levels, truncated, goals_used, goals_dropped, reserved)
    return r[0]


def box_occupied(mine, lo, ext):
    """occ[z, y, x] of the box [lo, lo + ext) of a region's minefield mine[z, y, x]: a cell is occupied iff its byte is 0."""
    return mine[lo[2]:lo[2] + ext[2], lo[1]:lo[1] + ext[1], lo[0]:lo[0] + ext[0]] == 0


def _merged(res0, standable, reached, levels, truncated, used, dropped):
    r = np.array(res0, dtype=RESULT_DTYPE).reshape(1).copy()
    w = lambda a, b: (int(a) + int(b)) & 0xFFFFFFFF
    r["standable"] = w(r["standable"][0], standable)
    r["reached"] = w(r["reached"][0], reached)
    r["truncated"] = w(r["truncated"][0], truncated)
    r["goals_used"] = w(r["goals_used"][0], used)
    r["goals_dropped"] = w(r["goals_dropped"][0], dropped)
    r["levels"] = max(int(r["levels"][0]), int(levels))
    return r[0]


# ---- the first restatement: the move graph and a queue -----------------------------------------------------------------------------
def build_graph(occ, p, goals, res0=None):
    ez, ey, ex = occ.shape
    lo, height = p["lo"], p["height"]
    big = 1 << 20

    def occupied(x, y, z):
        return True if z < 0 else (False if z >= ez else bool(occ[z, y, x]))

    def clear(x, y, z):
        n = 0
        while z + n < ez:
            if occ[z + n, y, x]:
                return n
            n += 1
        return big   # the cells above the box count as unoccupied

    stand = {}
    for z in range(ez):
        for y in range(ey):
            for x in range(ex):
                if not occ[z, y, x] and occupied(x, y, z - 1):
                    c = clear(x, y, z)
                    if c >= height:
                        stand[(x, y, z)] = c

    def moves(a):
        """(code, b) of the moves from a, in ORDER."""
        out = []
        for h, (dx, dy) in enumerate(STEPS_H):
            for k in range(p["max_climb"], -p["max_drop"] - 1, -1):
                b = (a[0] + dx, a[1] + dy, a[2] + k)
                if b not in stand:
                    continue
                lower = a if k >= 0 else b
                if stand[lower] >= abs(k) + height:
                    out.append((h | ((k + 8) << 2), b))
        return out

    out_moves = {a: moves(a) for a in stand}
    pred = collections.defaultdict(list)
    for a, ms in out_moves.items():
        for _, b in ms:
            pred[b].append(a)

    used = dropped = 0
    full = {}
    queue = collections.deque()
    for g in np.asarray(goals, dtype=np.int64).reshape(-1, 3):
        c = (int(g[0]) - lo[0], int(g[1]) - lo[1], int(g[2]) - lo[2])
        cell = None
        for s in range(p["goal_snap"] + 1):
            t = (c[0], c[1], c[2] - s)
            if 0 <= t[0] < ex and 0 <= t[1] < ey and 0 <= t[2] < ez and t in stand:
                cell = t
                break
        if cell is None:
            dropped += 1
            continue
        used += 1
        if cell not in full:
            full[cell] = 0
            queue.append(cell)
    while queue:
        b = queue.popleft()
        for a in pred[b]:
            if a not in full:
                full[a] = full[b] + 1
                queue.append(a)

    dist = np.full(occ.shape, UNREACHED, dtype=np.uint16)
    move = np.full(occ.shape, NO_MOVE, dtype=np.uint8)
    levels = 0
    for a, d in full.items():
        if d <= p["max_dist"]:
            dist[a[2], a[1], a[0]] = d
            levels = max(levels, d)
    for a, d in full.items():
        if 0 < d <= p["max_dist"]:
            move[a[2], a[1], a[0]] = next(code for code, b in out_moves[a] if full.get(b) == d - 1)
    truncated = int(any(d == p["max_dist"] + 1 for d in full.values()))
    reached = int(np.count_nonzero(dist != UNREACHED))
    return dist, move, _merged(result0() if res0 is None else res0, len(stand), reached, levels, truncated, used, dropped)


def sample_loop(dist, move, lo, agents):
    agents = np.asarray(agents, dtype=AGENT_DTYPE).reshape(-1)
    ez, ey, ex = dist.shape
    steps = np.zeros(len(agents), dtype=STEP_DTYPE)
    for i, a in enumerate(agents):
        pos = [float(v) for v in a["pos"]]
        bad = any(not np.isfinite(v) or abs(v) >= float(1 << 20) for v in pos) or any(int(v) != 0 for v in a["reserved"])
        bad = bad or int(a["snap_down"]) > 8 or int(a["snap_up"]) > 2
        if bad:
            steps[i] = ((-1, -1, -1), 0xFFFFFFFF, (-1, -1, -1), NO_MOVE)
            continue
        c0 = [int(np.floor(v)) for v in pos]
        zs = [c0[2] - s for s in range(int(a["snap_down"]) + 1)] + [c0[2] + s for s in range(1, int(a["snap_up"]) + 1)]
        steps[i] = (c0, 0xFFFFFFFF, c0, NO_MOVE)
        x, y = c0[0] - lo[0], c0[1] - lo[1]
        if not (0 <= x < ex and 0 <= y < ey):
            continue
        for tz in zs:
            z = tz - lo[2]
            if not 0 <= z < ez or dist[z, y, x] == UNREACHED:
                continue
            d, cell = int(dist[z, y, x]), (c0[0], c0[1], tz)
            if d == 0:
                steps[i] = (cell, 0, cell, NO_MOVE)
            else:
                m = int(move[z, y, x])
                dx, dy = STEPS_H[m & 3]
                steps[i] = (cell, d, (cell[0] + dx, cell[1] + dy, cell[2] + (m >> 2) - 8), m)
            break
    return steps


# ---- the second restatement: dilation with whole-array shifts ------------------------------------------------------------------------
def _shift(a, dx, dy, dz, fill):
    """s with s[z, y, x] = a[z + dz, y + dy, x + dx], `fill` where that lies outside."""
    s = np.full(a.shape, fill, dtype=a.dtype)
    ez, ey, ex = a.shape

    def span(d, n):
        return (slice(max(0, -d), max(0, min(n, n - d))), slice(max(0, d), max(0, min(n, n + d))))
    (tz, fz), (ty, fy), (tx, fx) = span(dz, ez), span(dy, ey), span(dx, ex)
    s[tz, ty, tx] = a[fz, fy, fx]
    return s


def build_dilate(occ, p, goals, res0=None):
    ez, ey, ex = occ.shape
    lo, height = np.asarray(p["lo"], dtype=np.int64), p["height"]
    free = ~occ
    # atleast[n][c]: CLEAR(c) >= n — an AND of the free cells going up, True above the box
    most = height + max(p["max_climb"], p["max_drop"])
    atleast = [np.ones(occ.shape, bool)]
    for n in range(1, most + 1):
        atleast.append(atleast[-1] & _shift(free, 0, 0, n - 1, True))
    stand = _shift(occ, 0, 0, -1, True) & atleast[height]

    # the goal cells: all candidates at once, the first standable one per record
    g = np.asarray(goals, dtype=np.int64).reshape(-1, 3) - lo
    front = np.zeros(occ.shape, bool)
    used = 0
    if len(g):
        zs = g[:, 2:3] - np.arange(p["goal_snap"] + 1)[None, :]
        inside = ((g[:, 0:1] >= 0) & (g[:, 0:1] < ex) & (g[:, 1:2] >= 0) & (g[:, 1:2] < ey) & (zs >= 0) & (zs < ez))
        ok = inside & stand[np.clip(zs, 0, ez - 1), np.clip(g[:, 1:2], 0, ey - 1), np.clip(g[:, 0:1], 0, ex - 1)]
        has = ok.any(axis=1)
        first = ok.argmax(axis=1)
        used = int(has.sum())
        front[zs[has, first[has]], g[has, 1], g[has, 0]] = True
    dropped = len(g) - used

    dist = np.full(occ.shape, UNREACHED, dtype=np.uint16)
    dist[front] = 0
    seen = front.copy()
    level, levels, truncated = 0, 0, 0
    while front.any():
        level += 1
        new = np.zeros(occ.shape, bool)
        for dx, dy in STEPS_H:
            for k in range(-p["max_drop"], p["max_climb"] + 1):
                there = _shift(front, dx, dy, k, False)
                lower = atleast[k + height] if k >= 0 else _shift(atleast[height - k], dx, dy, k, False)
                new |= there & lower
        new &= stand & ~seen
        if not new.any():
            break
        if level > p["max_dist"]:
            truncated = 1
            break
        dist[new] = level
        levels = level
        seen |= new
        front = new

    move = np.full(occ.shape, NO_MOVE, dtype=np.uint8)
    todo = (dist != UNREACHED) & (dist > 0)
    d32 = dist.astype(np.int64)
    for h, (dx, dy) in enumerate(STEPS_H):
        for k in range(p["max_climb"], -p["max_drop"] - 1, -1):
            nearer = _shift(d32, dx, dy, k, -7) == d32 - 1
            lower = atleast[k + height] if k >= 0 else _shift(atleast[height - k], dx, dy, k, False)
            hit = todo & nearer & lower
            move[hit] = h | ((k + 8) << 2)
            todo &= ~hit
    reached = int(np.count_nonzero(dist != UNREACHED))
    return dist, move, _merged(result0() if res0 is None else res0, int(stand.sum()), reached, levels, truncated, used, dropped)


def sample_array(dist, move, lo, agents):
    agents = np.asarray(agents, dtype=AGENT_DTYPE).reshape(-1)
    ez, ey, ex = dist.shape
    n = len(agents)
    pos = agents["pos"].astype(np.float64)
    with np.errstate(invalid="ignore"):
        good = np.isfinite(pos).all(axis=1) & (np.abs(pos) < 2.0 ** 20).all(axis=1) & (agents["reserved"] == 0).all(axis=1)
    good &= (agents["snap_down"] <= 8) & (agents["snap_up"] <= 2)
    c0 = np.where(good[:, None], np.floor(np.where(good[:, None], pos, 0.0)), -1).astype(np.int64)
    # candidate j of every agent: offsets 0, -1 .. -8, +1, +2, masked by the agent's ranges
    offs = np.array([0] + [-s for s in range(1, 9)] + [1, 2])
    allowed = np.concatenate([np.ones((n, 1), bool), np.arange(1, 9)[None, :] <= agents["snap_down"][:, None],
                              np.arange(1, 3)[None, :] <= agents["snap_up"][:, None]], axis=1)
    tz = c0[:, 2:3] + offs[None, :]
    x, y, z = c0[:, 0:1] - lo[0], c0[:, 1:2] - lo[1], tz - lo[2]
    inside = good[:, None] & allowed & (x >= 0) & (x < ex) & (y >= 0) & (y < ey) & (z >= 0) & (z < ez)
    idx = (np.clip(z, 0, ez - 1), np.clip(y, 0, ey - 1), np.clip(x, 0, ex - 1))
    d = np.where(inside, dist[idx], UNREACHED)
    found = (d != UNREACHED).any(axis=1)
    j = (d != UNREACHED).argmax(axis=1)
    rows = np.arange(n)
    steps = np.zeros(n, dtype=STEP_DTYPE)
    cell = c0.copy()
    cell[found, 2] = tz[rows, j][found]
    dd = d[rows, j].astype(np.int64)
    m = np.where(found & (dd > 0), move[idx][rows, j], NO_MOVE).astype(np.int64)
    step = np.zeros((n, 3), dtype=np.int64)
    walks = m != NO_MOVE
    h = m & 3
    step[:, 0] = np.where(walks, (h == 0).astype(np.int64) - (h == 1), 0)
    step[:, 1] = np.where(walks, (h == 2).astype(np.int64) - (h == 3), 0)
    step[:, 2] = np.where(walks, (m >> 2) - 8, 0)
    steps["cell"] = cell
    steps["dist"] = np.where(found, dd, 0xFFFFFFFF)
    steps["next"] = cell + step
    steps["move"] = m
    return steps


def follow(dist, move, start):
    """The cells (x, y, z) of the walk from `start` along the field's moves until dist is 0 (at most dist[start] + 1 of them)."""
    c = tuple(start)
    out = [c]
    for _ in range(int(dist[c[2], c[1], c[0]])):
        m = int(move[c[2], c[1], c[0]])
        if m == NO_MOVE:
            break
        dx, dy = STEPS_H[m & 3]
        c = (c[0] + dx, c[1] + dy, c[2] + (m >> 2) - 8)
        out.append(c)
    return out


# ---- the host's verdicts and plan (nav_check.hpp), restated -----------------------------------------------------------------------
HEAD_WORDS = 4112


def build_verdict(max_dist, height, max_climb, max_drop, goal_snap, reserved, goal_count, goals_null):
    """0 for a build the host accepts (the id and the box apart), 1 for one it refuses."""
    ok = (1 <= max_dist <= 4096 and 1 <= height <= 4 and 0 <= max_climb <= 2 and 0 <= max_drop <= 8 and 0 <= goal_snap <= 8 and
          not any(reserved) and goal_count <= 4096 and not (goal_count > 0 and goals_null))
    return 0 if ok else 1


def box_inside(lo, ext, R):
    return all(lo[k] >= 0 and lo[k] + ext[k] <= R for k in range(3))


def plan(ext, max_dist, levels):
    """(tiles_x, tiles_y, row_halves, bitmap_words, scratch_words, block_bytes, launches) of a field of `ext` and a build."""
    tx, ty = -(-ext[0] // 16), -(-ext[1] // 16)
    halves = tx + (tx & 1)
    bitmap = ext[1] * ext[2] * halves // 2
    scratch = HEAD_WORDS + 5 * bitmap
    launches = -(-(max_dist + 1) // levels) if max_dist else 0
    return tx, ty, halves, bitmap, scratch, scratch * 4 + 3 * ext[0] * ext[1] * ext[2], launches
