"""Expected values of hga_spanning_forest: Kruskal's loop with a plain dict union-find (the accepted positions
of union_find without a size cap or restricted ids, ReadClusteringEngine.cpp:424-489), a model of the
device's Borůvka rounds (the rounds and the depth of the pointer forest a round's hooks leave), and the
edge lists the CPU and GPU tests share.  Every id is a ReadID of FIRST_ID .. FIRST_ID + N_READS - 1."""
import functools

import numpy as np

import pyref_cluster as pc

FIRST_ID = 700
N_READS = 5000


def kruskal(x, y):
    """The ascending positions i at which x[i] and y[i] are in two components."""
    parent = {}

    def find(v):
        r = parent.setdefault(v, v)
        while parent[r] != r:
            r = parent[r]
        while parent[v] != r:
            parent[v], v = r, parent[v]
        return r

    out = []
    for i, (a, b) in enumerate(zip(np.asarray(x).tolist(), np.asarray(y).tolist())):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[ra] = rb
            out.append(i)
    return out


def boruvka_model(x, y):
    """(accepted positions ascending, rounds that hook, the largest depth of the pointer forest right after a
    round's hooks): per round every component takes its smallest live position; of two components that
    took the same one the smaller id stays a root, every other one points at the component across."""
    x, y = np.asarray(x).tolist(), np.asarray(y).tolist()
    comp = {v: v for v in set(x) | set(y)}
    live, acc, rounds, deepest = list(range(len(x))), [], 0, 0
    while True:
        best, kept = {}, []
        for i in live:
            cx, cy = comp[x[i]], comp[y[i]]
            if cx == cy:
                continue
            kept.append(i)
            for c in (cx, cy):
                if best.get(c, i + 1) > i:
                    best[c] = i
        if not kept:
            return sorted(acc), rounds, deepest
        rounds += 1
        up = {}
        for c, e in best.items():
            cx, cy = comp[x[e]], comp[y[e]]
            other = cy if cx == c else cx
            if best.get(other) == e and c < other:
                continue
            up[c] = other
            acc.append(e)
        depth = {}
        for c in up:
            path = []
            while c in up and c not in depth:
                path.append(c)
                c = up[c]
            d = depth.get(c, 0)
            for p in reversed(path):
                d += 1
                depth[p] = d
        deepest = max(deepest, max(depth.values()))
        roots = {}
        for c in sorted(set(comp.values()), key=lambda c: depth.get(c, 0)):   # a parent before its children
            roots[c] = roots[up[c]] if c in up else c
        comp = {v: roots[c] for v, c in comp.items()}
        live = kept


def replay(x, y, positions, min_size):
    """pyref_cluster.union_find over the connections at `positions` only."""
    x, y = np.asarray(x).tolist(), np.asarray(y).tolist()
    return pc.union_find([(x[i], y[i], 0) for i in positions], set(), min_size, -1)


def full(x, y, min_size):
    """pyref_cluster.union_find over the whole list, less the one thing a replay cannot give: the one-vertex
    component of an id that occurs in self-loops only (never accepted, so the replay never sees the id; it
    is returned at min_size <= 1 alone, and get_connections lists no self-loop, :316).  An id with any other
    connection is in an accepted one: before its first such connection it is alone in its component."""
    x, y = np.asarray(x).tolist(), np.asarray(y).tolist()
    other = {v for a, b in zip(x, y) if a != b for v in (a, b)}
    out = pc.union_find(list(zip(x, y, [0] * len(x))), set(), min_size, -1)
    return [(comp, tree) for comp, tree in out if tree or comp[0] in other]


def _ids(pairs):
    a = np.asarray(pairs, np.int64).reshape(-1, 2) + FIRST_ID
    return a[:, 0].astype(np.uint32), a[:, 1].astype(np.uint32)


def _clique(lo, n):
    return [(lo + i, lo + j) for i in range(n) for j in range(i + 1, n)]


def _random(seed, n_vertices=3000, n_edges=20000):
    rng = np.random.default_rng(seed)
    return rng.integers(0, n_vertices, (n_edges, 2)).tolist()   # self-loops and repeats as they fall


@functools.lru_cache(maxsize=None)
def shapes():
    """name -> (x, y) as uint32 ReadID arrays."""
    chain = [(i, i + 1) for i in range(4096)]
    low = lambda v: v & -v
    halving = sorted(chain, key=lambda e: (low(e[1]), e[0]))
    some = [(3, 9), (9, 4), (4, 3), (20, 21), (9, 20), (21, 3), (40, 41)]
    cross = [(a, 64 + b) for a in range(64) for b in range(64)]
    two = _clique(0, 64) + _clique(64, 64)
    rnd = {seed: _random(seed) for seed in (1, 2, 3)}
    perm = np.random.default_rng(9).permutation(N_READS)
    out = {
        "empty": [],
        "one": [(5, 2)],
        "self_loops": [(v, v) for v in (0, 7, 7, 4999)],
        "doubled": [e for a, b in some for e in ((a, b), (b, a), (a, b))],
        "chain": chain,
        "halving": halving,
        "cliques_join_last": two + [(63, 64)],
        "cliques_cross_first": cross + two,
        "cliques_cross_last": two + cross,   # round 1: 4096 live edges, every offer to one of two words
        "isolated": [(10, 4000), (4000, 4999), (11, 10), (4999, 11)],   # four of the 5000 vertices
    }
    for n in (64, 65, 4097):
        out[f"star_x_{n}"] = [(0, v) for v in range(1, n)]
        out[f"star_y_{n}"] = [(v, 2) for v in range(n) if v != 2]
    for seed, edges in rnd.items():
        out[f"random_{seed}"] = edges
    out["random_1_permuted"] = [(int(perm[a]), int(perm[b])) for a, b in rnd[1]]
    return {name: _ids(edges) for name, edges in out.items()}


@functools.lru_cache(maxsize=None)
def expected(name):
    return kruskal(*shapes()[name])


@functools.lru_cache(maxsize=None)
def model(name):
    return boruvka_model(*shapes()[name])


def check_not_hollow():
    """Each shape has the property it exists for."""
    s = shapes()
    n = lambda name: len(s[name][0])
    for x, y in s.values():
        both = np.concatenate([x, y]).astype(np.int64)
        assert len(both) == 0 or (both.min() >= FIRST_ID and both.max() < FIRST_ID + N_READS)
    assert expected("empty") == [] and expected("one") == [0] and expected("self_loops") == []
    # repeats in both directions: only first occurrences, and not all of those (the triangle's third edge)
    assert expected("doubled") == [0, 3, 9, 12, 18] and n("doubled") == 21
    # the ascending chain: every edge in one round, hooked into one path
    assert model("chain") == (list(range(4096)), 1, 4096)
    # the halving chain: every edge again, but a round only joins neighbours pairwise
    acc, rounds, depth = model("halving")
    assert acc == list(range(4096)) and rounds == 12 and depth <= 2
    for c in (64, 65, 4097):   # one wave, one wave and a lane, many workgroups: every offer to one word
        for side in "xy":
            acc, rounds, depth = model(f"star_{side}_{c}")
            assert acc == list(range(c - 1)) and rounds == 1 and depth <= 2
    e = expected("cliques_join_last")
    assert len(e) == 127 and e[-1] == n("cliques_join_last") - 1 and model("cliques_join_last")[1] == 2
    e = expected("cliques_cross_first")   # the cross edges alone span everything; the cliques add nothing
    assert len(e) == 127 and e[-1] < 4096 and e[:64] == list(range(64))
    e = expected("cliques_cross_last")
    assert len(e) == 127 and e[-1] == 2 * 2016 and model("cliques_cross_last")[1] == 2
    for name in ("random_1", "random_2", "random_3", "random_1_permuted"):
        acc, rounds, _ = model(name)
        assert 2900 < len(acc) < 3000 and rounds >= 4 and n(name) > 6 * len(acc)
        assert (s[name][0] == s[name][1]).sum() >= 1
    assert expected("random_1_permuted") == expected("random_1") != expected("random_2")
    assert expected("isolated") == [0, 1, 2]
