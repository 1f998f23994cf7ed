"""The rules of the navigation fields without a GPU: the two restatements of tests/nav_field_ref.py (a move graph with a queue;
dilation with whole-array shifts) agree on dist, move, the result record and the sampled steps for every named case of
tests/nav_field_sets.py, and every case does what its name says."""
import numpy as np
import pytest

from tests import nav_field_ref as ref
from tests import nav_field_sets as sets

CASES = sets.placed(dict(sets.cases(), **sets.big_cases()))
RES0 = ref.result0(0xFFFFFFF0, 0xFFFFFFFE, 5, 0xFFFFFFFF, 0xFFFFFFFD, 7, (11, 13))


@pytest.fixture(scope="module")
def built():
    out = {}
    for name, c in CASES.items():
        p, goals = sets.params_of(c), sets.goals_of(c)
        out[name] = (ref.build_graph(c["occ"], p, goals, RES0), ref.build_dilate(c["occ"], p, goals, RES0))
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_the_two_restatements_agree(name, built):
    a, b = built[name]
    assert np.array_equal(a[0], b[0]), "dist"
    assert np.array_equal(a[1], b[1]), "move"
    assert a[2].tobytes() == b[2].tobytes(), (a[2], b[2])
    c = CASES[name]
    for agents in (sets.every_cell_agents(c["lo"], sets.ext_of(c), 1, 1), sets.odd_agents(c["lo"], sets.ext_of(c))):
        assert ref.sample_loop(a[0], a[1], c["lo"], agents).tobytes() == ref.sample_array(a[0], a[1], c["lo"], agents).tobytes()


@pytest.mark.parametrize("name", list(CASES))
def test_a_case_does_what_its_name_says(name, built):
    c = CASES[name]
    dist, move, res = built[name][0]
    assert c["expect"]
    for (x, y, z), want in c["expect"]:
        d = int(dist[z, y, x])
        if want == "reached":
            assert d != ref.UNREACHED, (x, y, z)
        elif want == "unreached":
            assert d == ref.UNREACHED and move[z, y, x] == ref.NO_MOVE, (x, y, z)
        else:
            assert d == want, ((x, y, z), d, want)
    for key, field in (("truncated", "truncated"), ("used", "goals_used"), ("dropped", "goals_dropped")):
        if key in c["p"]:
            assert (int(res[field]) - int(RES0[field])) & 0xFFFFFFFF == c["p"][key], key
    assert res["reserved"].tolist() == [11, 13] and int(res["levels"]) == max(5, int(dist[dist != ref.UNREACHED].max(initial=0)))
    # the goals have no move, every other reached cell has one, and following the moves counts dist down to a goal
    reached = dist != ref.UNREACHED
    assert np.array_equal(move != ref.NO_MOVE, reached & (dist > 0))
    for z, y, x in np.argwhere(reached)[::7]:
        walk = ref.follow(dist, move, (x, y, z))
        assert len(walk) == int(dist[z, y, x]) + 1 and dist[walk[-1][2], walk[-1][1], walk[-1][0]] == 0


def test_the_cases_cover_what_the_device_can_get_wrong():
    c = CASES
    assert sets.ext_of(c["two tiles wide"])[0] == 17
    dist = ref.build_dilate(c["serpentine maze re-enters tiles"]["occ"], sets.params_of(c["serpentine maze re-enters tiles"]),
                            sets.goals_of(c["serpentine maze re-enters tiles"]))[0]
    # the way crosses the tile border x = 15 | 16 once per corridor: more often than G, and it is longer than 3 G
    crossings = sum(1 for y in range(0, 21, 2) if dist[1, y, 15] != ref.UNREACHED and dist[1, y, 16] != ref.UNREACHED)
    assert crossings == 11 > sets.G and int(dist[dist != ref.UNREACHED].max()) == 449 > 3 * sets.G
    assert c["max_dist a multiple of G"]["p"]["max_dist"] % sets.G == 0 and c["max_dist no multiple of G"]["p"]["max_dist"] % sets.G != 0
    assert any(l % 2 for cc in c.values() for l in cc["lo"]) and c["the region's far corner"]["lo"] == (237, 238, 251)
    assert sets.ext_of(c["z extent 256 on a 20 x 20 footprint"]) == (20, 20, 256)
    for name, cc in c.items():
        if name not in sets.big_cases():
            ex, ey, ez = sets.ext_of(cc)
            assert ex <= 48 and ey <= 48 and ez <= 24, name
    # every move code of the default parameters occurs in the every-cell sample of one case or another
    codes = set()
    for name in ("stairs of rise 1 under max_climb 1", "cliff of 3 under max_drop 3", "several goals"):
        codes |= set(np.unique(ref.build_dilate(c[name]["occ"], sets.params_of(c[name]), sets.goals_of(c[name]))[1]).tolist())
    assert {h | (8 << 2) for h in range(4)} <= codes and (0 | (9 << 2)) in codes and (0 | (5 << 2)) in codes


def test_the_world_holds_every_case_apart():
    mats, mine = sets.world(CASES)
    for name, c in CASES.items():
        assert np.array_equal(ref.box_occupied(mine, c["lo"], sets.ext_of(c)), c["occ"]), name
