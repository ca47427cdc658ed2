"""Expected values of hga_spanning_forest_restricted: the loop of union_find without a size cap
(ReadClusteringEngine.cpp:452-480) restated with a plain dict and a per-root flag, which is what every test
compares against; the contraction the device relies on (all restricted ids renamed to the smallest one, then
forest_ref's model of the Borůvka rounds), which the CPU tests compare against the loop, never against
itself; and the cases the CPU and GPU tests share, on forest_ref's vertex range."""
import collections
import functools

import numpy as np

import forest_ref as fr
import pyref_cluster as pc

FIRST_ID, N_READS = fr.FIRST_ID, fr.N_READS


def kruskal_restricted(x, y, restricted, by_rule=None):
    """The ascending positions i at which x[i] and y[i] are in two components that do not both hold a
    restricted id.  by_rule: a list that receives the positions rejected by that second rule alone."""
    restricted = set(np.asarray(restricted, np.int64).tolist())
    parent, holds = {}, {}

    def find(v):
        if v not in parent:
            parent[v] = v
            holds[v] = v in restricted
        r = v
        while parent[r] != r:
            r = parent[r]
        while parent[v] != r:
            parent[v], v = r, parent[v]
        return r

    out = []
    for i, (a, b) in enumerate(zip(np.asarray(x).tolist(), np.asarray(y).tolist())):
        ra, rb = find(a), find(b)
        if ra == rb:
            continue
        if holds[ra] and holds[rb]:
            if by_rule is not None:
                by_rule.append(i)
            continue
        parent[ra] = rb
        holds[rb] = holds[rb] or holds[ra]
        out.append(i)
    return out


def contracted_model(x, y, restricted):
    """forest_ref.boruvka_model on the list with every restricted id renamed to the smallest one: (accepted
    positions, rounds that hook, the deepest pointer forest).  What the device computes."""
    r = np.unique(np.asarray(restricted, np.int64))
    x, y = np.asarray(x, np.int64).copy(), np.asarray(y, np.int64).copy()
    if len(r):
        x[np.isin(x, r)] = r[0]
        y[np.isin(y, r)] = r[0]
    return fr.boruvka_model(x, y)


def replay(x, y, positions, restricted, min_size):
    """pyref_cluster.union_find over the connections at `positions` only, with the restricted set."""
    x, y = np.asarray(x).tolist(), np.asarray(y).tolist()
    return pc.union_find([(x[i], y[i], 0) for i in positions], set(np.asarray(restricted).tolist()), min_size, -1)


def full(x, y, positions, restricted, min_size):
    """pyref_cluster.union_find over the whole list, less the one thing a replay cannot give: the one-member
    component of an id that is in no accepted connection (`positions`), returned at min_size <= 1 alone."""
    x, y = np.asarray(x).tolist(), np.asarray(y).tolist()
    seen = {v for i in positions for v in (x[i], y[i])}
    out = pc.union_find(list(zip(x, y, [0] * len(x))), set(np.asarray(restricted).tolist()), min_size, -1)
    return [(comp, tree) for comp, tree in out if tree or comp[0] in seen]


# x, y: uint32 ReadIDs; restricted: uint32 ReadIDs as handed to the call (any order, repeats as they are);
# the call works on entries [first, first + count) of the list (count None: to the end)
Case = collections.namedtuple("Case", "x y restricted first count")

HUBS = tuple(range(8))                   # vertices (id - FIRST_ID) of the hubs cases
HUB_LEAF0 = 1000                         # their leaves: HUB_LEAF0 .. HUB_LEAF0 + leaves - 1
HUB_SIZES = {"hubs_9": (9, 4), "hubs_300": (300, 100), "hubs": (600, 500)}   # name -> (leaves, leaf-leaf edges)
WINDOWS = ((0, 0), (0, 1), (1, None), (5, 2048), (2049, 7000), (0, 2049), (19900, 1000), (20000, 5), (20009, 1))


def _rid(vertices):
    return (np.asarray(vertices, np.int64) + FIRST_ID).astype(np.uint32)


def _hubs(leaves, n_leaf_leaf, seed):
    """Every leaf meets every hub in a shuffled order, either end first; every hub-hub edge anywhere; leaf-leaf
    edges after both leaves met their first hubs, which differ.  -> (edges, kinds): kind 0 a leaf's first hub
    edge, 1 a later hub-leaf edge, 2 hub-hub, 3 leaf-leaf."""
    rng = np.random.default_rng(seed)
    hl = [(h, HUB_LEAF0 + l) for h in HUBS for l in range(leaves)]
    hl = [hl[i] for i in rng.permutation(len(hl))]
    first = {}
    for p, (h, l) in enumerate(hl):
        first.setdefault(l, (p, h))
    items = [(p, 1, (h, l), 0 if first[l][0] == p else 1) for p, (h, l) in enumerate(hl)]
    for a in HUBS:
        for b in HUBS:
            if a < b:   # before hub-leaf edge p
                items.append((int(rng.integers(0, len(hl) + 1)), 0, (a, b), 2))
    made = 0
    while made < n_leaf_leaf:
        a, b = (HUB_LEAF0 + int(v) for v in rng.integers(0, leaves, 2))
        if a == b or first[a][1] == first[b][1]:
            continue
        after = max(first[a][0], first[b][0]) + 1
        items.append((int(rng.integers(after, len(hl) + 1)), 0, (a, b), 3))
        made += 1
    items.sort(key=lambda t: (t[0], t[1]))   # (stable: inserted edges before the hub-leaf edge of their place)
    flip = rng.integers(0, 2, len(items)).tolist()
    edges = [e[::-1] if f else e for (_, _, e, _), f in zip(items, flip)]
    return edges, [k for _, _, _, k in items]


@functools.lru_cache(maxsize=None)
def hub_kinds(name):
    return _hubs(*HUB_SIZES[name], seed=31)[1]


@functools.lru_cache(maxsize=None)
def cases():
    """name -> Case."""
    s = fr.shapes()
    everyone = np.arange(FIRST_ID, FIRST_ID + N_READS, dtype=np.uint32)
    rng = np.random.default_rng(5)
    some3000 = _rid(np.sort(rng.choice(3000, 150, replace=False)))   # 5 % of the vertices of forest_ref's random lists
    out = {
        "random_1_none": Case(*s["random_1"], _rid([]), 0, None),
        "random_1_single": Case(*s["random_1"], _rid([int(s["random_1"][0][0]) - FIRST_ID]), 0, None),
        "random_2_everyone": Case(*s["random_2"], everyone, 0, None),
        "one_everyone": Case(*s["one"], everyone[::-1].copy(), 0, None),
        "chain_ends": Case(*s["chain"], _rid([0, 4096]), 0, None),
        "halving_ends": Case(*s["halving"], _rid([4096, 0]), 0, None),
        "chain_mid": Case(*s["chain"], _rid([0, 2048]), 0, None),
        "halving_mid": Case(*s["halving"], _rid([2048, 0]), 0, None),
        "cliques_join_last": Case(*s["cliques_join_last"], _rid([5, 64 + 7]), 0, None),
        "cliques_cross_last": Case(*s["cliques_cross_last"], _rid([0, 64]), 0, None),
        "random_3_some": Case(*s["random_3"], some3000, 0, None),
        # restricted ids no edge names, the smallest ReadID among them: R is a vertex without an edge
        "isolated_unused": Case(*s["isolated"], _rid([2500, 0, 1, N_READS - 2]), 0, None),
        # ... and R without an edge while two restricted ids have some
        "isolated_r_unused": Case(*s["isolated"], _rid([4999, 0, 10]), 0, None),
        "doubled_repeats": Case(*s["doubled"], _rid([3, 20, 3, 20, 20, 40, 3]), 0, None),
    }
    for name, (leaves, ll) in HUB_SIZES.items():
        edges, _ = _hubs(leaves, ll, seed=31)
        a = _rid(edges)
        out[name] = Case(a[:, 0].copy(), a[:, 1].copy(), _rid(HUBS), 0, None)
    for j, (first, count) in enumerate(WINDOWS):
        out[f"random_1_window_{j}"] = Case(*s["random_1"], some3000, first, count)
    return out


def window(case):
    n = len(case.x)
    a = min(case.first, n)
    return a, n if case.count is None else min(n, a + case.count)


@functools.lru_cache(maxsize=None)
def expected(name):
    """(the absolute accepted positions of the case, the absolute positions the restricted rule rejected)."""
    c = cases()[name]
    a, b = window(c)
    by_rule = []
    acc = kruskal_restricted(c.x[a:b], c.y[a:b], c.restricted, by_rule)
    return [a + p for p in acc], [a + p for p in by_rule]


@functools.lru_cache(maxsize=None)
def model(name):
    c = cases()[name]
    a, b = window(c)
    acc, rounds, depth = contracted_model(c.x[a:b], c.y[a:b], c.restricted)
    return [a + p for p in acc], rounds, depth


def check_not_hollow():
    """Each case has the property it exists for."""
    cs = cases()
    for c in cs.values():
        ids = np.concatenate([c.x, c.y, c.restricted]).astype(np.int64)
        assert ids.min() >= FIRST_ID and ids.max() < FIRST_ID + N_READS
    n = lambda name: len(cs[name].x)
    plain = lambda name: fr.kruskal(cs[name].x, cs[name].y)
    # no restricted id, and one: nothing is rejected by the rule
    assert len(cs["random_1_none"].restricted) == 0 and len(cs["random_1_single"].restricted) == 1
    for name in ("random_1_none", "random_1_single"):
        assert expected(name) == (fr.expected("random_1"), [])
    # every vertex restricted: nothing is accepted, all but the self-loops by the rule
    for name, base in (("random_2_everyone", "random_2"), ("one_everyone", "one")):
        acc, rule = expected(name)
        x, y = cs[name].x, cs[name].y
        assert acc == [] and len(rule) == int((x != y).sum()) > 0 and fr.expected(base)
    # two vertices of the chain restricted: the connection that would close the path between them is rejected,
    # all others are accepted.  Between the two ends that is the last connection of the list in either order
    # (every edge is on the path; both orders end with (4095, 4096)); between 0 and 2048 it is the last edge of
    # the path's 2048, whose position depends on the order.
    for ends, mid in (("chain_ends", "chain_mid"), ("halving_ends", "halving_mid")):
        for name in (ends, mid):
            acc, rule = expected(name)
            assert len(rule) == 1 and acc == [p for p in range(4096) if p != rule[0]]
        assert expected(ends)[1] == [4095]
    assert expected("chain_mid")[1] == [2047] and expected("halving_mid")[1] == [4094]
    assert model("chain_ends")[1] == 1 and model("halving_ends")[1] >= 10 and model("halving_mid")[1] >= 10
    acc, rule = expected("cliques_join_last")
    assert len(acc) == 126 and rule == [n("cliques_join_last") - 1] and len(plain("cliques_join_last")) == 127
    acc, rule = expected("cliques_cross_last")   # the cliques form, then no cross edge may join them
    assert len(acc) == 126 and rule == list(range(2 * 2016, n("cliques_cross_last"))) and len(rule) == 4096
    # hubs: round 0 offers every edge to the one word best[R]
    for name, (leaves, ll) in HUB_SIZES.items():
        kinds = hub_kinds(name)
        acc, rule = expected(name)
        assert [kinds.count(k) for k in range(4)] == [leaves, 7 * leaves, 28, ll]
        assert acc == [p for p, k in enumerate(kinds) if k == 0]
        assert set(rule) >= {p for p, k in enumerate(kinds) if k >= 2}   # hub-hub and leaf-leaf: by the rule
        assert model(name)[1] <= 2
        hub_ids = set(cs[name].restricted.tolist())
        assert all((int(a) in hub_ids) != (int(b) in hub_ids)
                   for a, b, k in zip(cs[name].x, cs[name].y, kinds) if k < 2)
    assert 64 < 8 * 9 < 2048 < 8 * 300 < 2 * 2048 < 8 * 600   # a wave, a workgroup's 2048 edges, several of those
    acc, rule = expected("random_3_some")
    assert len(cs["random_3_some"].restricted) == 150 and len(rule) >= 1 and acc != fr.expected("random_3")
    assert len(acc) < len(fr.expected("random_3"))
    # restricted ids without an edge change nothing; R = the first vertex has no edge in either case
    used = set(np.concatenate(fr.shapes()["isolated"]).tolist())
    c = cs["isolated_unused"]
    assert not used & set(c.restricted.tolist()) and c.restricted.min() == FIRST_ID
    assert expected("isolated_unused") == (fr.expected("isolated"), []) and fr.expected("isolated") == [0, 1, 2]
    c = cs["isolated_r_unused"]
    assert c.restricted.min() == FIRST_ID and FIRST_ID not in used and len(used & set(c.restricted.tolist())) == 2
    assert expected("isolated_r_unused") == ([0, 2], [1, 3])
    c = cs["doubled_repeats"]
    assert len(c.restricted) > len(set(c.restricted.tolist())) == 3
    assert expected("doubled_repeats") == ([0, 3, 9, 18], [12, 13, 14, 15, 16, 17])
    assert expected("doubled_repeats")[0] != fr.expected("doubled")
    # windows: absolute positions, and at least one window starts past an accepted position of the whole list
    whole = kruskal_restricted(cs["random_1_window_0"].x, cs["random_1_window_0"].y, cs["random_1_window_0"].restricted)
    total = n("random_1_window_0")
    assert total == 20000
    past = 0
    for j, (first, count) in enumerate(WINDOWS):
        acc, rule = expected(f"random_1_window_{j}")
        a, b = window(cs[f"random_1_window_{j}"])
        assert all(a <= p < b for p in acc + rule)
        assert bool(acc) == (first < total and count != 0)
        if acc and whole[0] < a:
            past += 1
            assert acc[0] >= a and acc != [p for p in whole if a <= p < b]   # the forest of the slice, not a slice
    assert past >= 3 and any(expected(f"random_1_window_{j}")[1] for j in range(len(WINDOWS)))
