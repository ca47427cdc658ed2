"""Expected values of hga_tree_tails: get_spanning_tree_tails
(src/clustering/ReadClusteringEngine.cpp:509-573) restated on plain Python ints modulo 2^64 under the
project's fixed orders (host/clustering.h "Determinism": the first start is the smallest id, the farthest
vertex is the one at the largest distance with the smallest id, lists ascend), and the forests the CPU and
GPU tests share.  Every builder asserts that what it built is not hollow."""
import functools
from collections import deque

import numpy as np

M = 1 << 64


class TreeRef:
    """One tree's result: left / right (ascending ids), ends = (right_id, right_dist, left_id, left_dist),
    starts = the start vertices of the three passes, and what the passes met on the way."""

    def __init__(self, tree, ov, length, tail):
        self.left, self.right, self.ends, self.starts = [], [], (0, 0, 0, 0), ()
        self.tie = self.wrapped = False
        adj = {}
        for (a, b), d in zip(tree, ov):
            adj.setdefault(a, {}).setdefault(b, int(d))
            adj.setdefault(b, {}).setdefault(a, int(d))
        if not adj:
            return

        def bfs(start):
            q, seen, dist = deque([start]), {start}, {start: int(length[start]) % M}
            while q:
                v = q.popleft()
                for a, d in adj[v].items():
                    if a not in seen:
                        seen.add(a)
                        raw = dist[v] + int(length[a]) - d
                        self.wrapped |= not 0 <= raw < M
                        dist[a] = raw % M
                        q.append(a)
            return dist

        def far(dist):
            mx = max(dist.values())
            at = sorted(v for v, d in dist.items() if d == mx)
            self.tie |= len(at) > 1
            return at[0], mx

        s0 = min(adj)
        f, _ = far(bfs(s0))
        dr = bfs(f)
        fr, frd = far(dr)
        self.right = [v for v in sorted(dr) if (dr[v] + tail) % M > frd]
        dl = bfs(fr)
        fl, fld = far(dl)
        self.left = [v for v in sorted(dl) if (dl[v] + tail) % M > fld]
        self.ends = (fr, frd, fl, fld)
        self.starts = (s0, f, fr)


def tree_tails(trees, overlap, length, tail):
    """trees: edge lists; overlap: one int per edge in the trees' order; length: by id.  A list of TreeRef."""
    out, at = [], 0
    for tree in trees:
        out.append(TreeRef(tree, overlap[at:at + len(tree)], length, tail))
        at += len(tree)
    return out


# ---- shapes: edges over local vertex numbers 0 .. n - 1
def path(n_edges):
    return [(i, i + 1) for i in range(n_edges)]


def star(n_vertices):
    return [(0, i) for i in range(1, n_vertices)]


def caterpillar(spine, legs):
    e = path(spine - 1)
    nxt = spine
    for s in range(spine):
        for _ in range(legs if s % 3 else 0):
            e.append((s, nxt))
            nxt += 1
    return e


def random_tree(n_vertices, rng):
    return [(int(rng.integers(0, v)), v) for v in range(1, n_vertices)]


class Forest:
    """Trees over ids scattered through [first_id, first_id + n_reads) and interleaved between the trees,
    the edges of a tree shuffled and given in both orientations."""

    def __init__(self, shapes, first_id, n_reads, seed):
        rng = np.random.default_rng(seed)
        total = sum((max(max(e) for e in s) + 1) if s else 0 for s in shapes)
        assert total <= n_reads
        pool = first_id + rng.permutation(n_reads)[:total]
        self.first_id, self.n_reads = first_id, n_reads
        self.trees, at = [], 0
        for s in shapes:
            nv = (max(max(e) for e in s) + 1) if s else 0
            ids = pool[at:at + nv]
            at += nv
            edges = [(int(ids[a]), int(ids[b])) if rng.integers(0, 2) else (int(ids[b]), int(ids[a])) for a, b in s]
            self.trees.append([edges[i] for i in rng.permutation(len(edges))])
        self.n_edges = sum(len(t) for t in self.trees)
        spans = [(min(min(e) for e in t), max(max(e) for e in t)) for t in self.trees if t]
        # interleaved: some tree's id range contains an id of another tree; both orientations occur
        assert any(a[0] < b[0] < a[1] for a in spans for b in spans if a is not b)
        flat = [e for t in self.trees for e in t]
        assert any(a < b for a, b in flat) and any(a > b for a, b in flat)


class Weights:
    """Read lengths (uint32, by id - first_id) and per-edge overlaps (int32) of one arithmetic kind."""

    def __init__(self, forest, kind, seed):
        rng = np.random.default_rng(seed)
        n, E = forest.n_reads, forest.n_edges
        if kind == "plain":      # overlaps below the lengths: nothing wraps
            self.length = rng.integers(2000, 30000, n).astype(np.uint32)
            self.overlap = rng.integers(0, 2000, E).astype(np.int32)
        elif kind == "equal":    # every step adds the same: many vertices tie for farthest
            self.length = np.full(n, 5000, np.uint32)
            self.overlap = np.full(E, 1200, np.int32)
        elif kind == "wrap":     # overlaps beyond dist + length: distances pass below zero
            self.length = rng.integers(50, 400, n).astype(np.uint32)
            self.overlap = rng.integers(0, 3000, E).astype(np.int32)
        elif kind == "negative":
            self.length = rng.integers(100, 3000, n).astype(np.uint32)
            self.overlap = rng.integers(-2500, 2500, E).astype(np.int32)
        else:
            raise ValueError(kind)
        self.kind = kind
        self.by_id = {forest.first_id + i: int(l) for i, l in enumerate(self.length)}


FIRST_ID, N_READS = 7, 40_000
TAILS = (0, 1, 1 << 63, M - 1)


@functools.lru_cache(maxsize=None)
def shapes_forest():
    """The shapes of the issue in one call: 0 and 1 edges, a star of 65 vertices, paths on either side of
    the pointer-jumping round boundaries (2 * 32 = 2^6, 2 * 1024 = 2^11), a deep path, a caterpillar, a
    random tree of 5000 vertices."""
    rng = np.random.default_rng(5)
    shapes = [[], path(1), star(65), path(31), [], path(32), path(33), path(1023), path(1024), path(1025), path(3000),
              caterpillar(120, 2), random_tree(5000, rng), path(2), []]
    return Forest(shapes, FIRST_ID, N_READS, 6)


@functools.lru_cache(maxsize=None)
def random_forest():
    """300 random trees of 1-200 edges."""
    rng = np.random.default_rng(9)
    return Forest([random_tree(int(rng.integers(2, 202)), rng) for _ in range(300)], FIRST_ID, N_READS, 10)


@functools.lru_cache(maxsize=None)
def weights(which, kind):
    return Weights(shapes_forest() if which == "shapes" else random_forest(), kind, 11)


@functools.lru_cache(maxsize=None)
def expected(which, kind, tail):
    f = shapes_forest() if which == "shapes" else random_forest()
    w = weights(which, kind)
    return tree_tails(f.trees, w.overlap.tolist(), w.by_id, tail)


def merged_trees(ref, no):
    """Spanning trees over ids of a tests/tailsets_ref.py case after merge step `no`, merge survivors
    included: a star around a survivor, a path with a survivor inside, a random tree with survivors and the
    read without hits.  Returns (trees, the edges' overlaps on that step's lists by tests/pyref_cluster.py)."""
    c = ref.c
    eng = c.steps[no].engine()
    eng.pos = c.eng.pos   # positions belong to the reads: merges never change them
    sv = [int(i) for i in c.all_survivors(no)]
    touched = {i for s in c.steps[:no + 1] for g in s.groups if len(g) >= 2 for i in g}
    others = [i for i in c.ids if i not in touched]
    rng = np.random.default_rng(3 + no)
    pick = [int(i) for i in rng.permutation(others)[:90]]
    a, b, d = pick[:30], sorted(pick[30:60]), pick[60:90] + [int(ref.no_hit)] + sv[2:6]
    centre = sv[0] if sv else a.pop()
    if len(sv) > 1:
        b.insert(15, sv[1])
    trees = [[(centre, v) if i % 2 else (v, centre) for i, v in enumerate(a)],
             [(b[i + 1], b[i]) if i % 3 else (b[i], b[i + 1]) for i in range(len(b) - 1)],
             [],
             [(d[int(rng.integers(0, v))], d[v]) for v in range(1, len(d))]]
    ov = [eng.overlap(x, y) if x in eng.comps and y in eng.comps else 0 for t in trees for x, y in t]
    assert sum(o > 0 for o in ov) >= 5, (c.name, no, ov)
    if sv:   # edges at a survivor answer on its union
        at = [o for (x, y), o in zip([e for t in trees for e in t], ov) if x in sv or y in sv]
        assert len(at) >= 20 and sum(o > 0 for o in at) >= 5, (c.name, no, at)
    return trees, ov


def check_not_hollow():
    """What the cases must contain for the tests to mean something."""
    avg_tail = 20000
    plain = expected("shapes", "plain", avg_tail)
    assert any(len(set(r.starts)) == 3 for r in plain)                   # three passes, three start vertices
    assert any(0 < len(r.left) < len(r.starts) + 3000 and r.left != r.right for r in plain)
    assert not any(r.wrapped for r in plain)
    equal = expected("shapes", "equal", avg_tail)
    assert sum(r.tie for r in equal) >= 3                                 # a distance tie decided by id
    assert equal[2].tie and len(shapes_forest().trees[2]) == 64           # the star: every leaf ties
    assert any(r.wrapped for r in expected("shapes", "wrap", avg_tail))  # a wrapped distance
    assert any(r.wrapped for r in expected("shapes", "negative", avg_tail))
    assert any(d >= 1 << 63 for r in expected("shapes", "wrap", avg_tail) for d in (r.ends[1], r.ends[3]))
    for r, t in zip(plain, shapes_forest().trees):   # a tree without edges gives nothing, any other both ends
        assert (r.left == [] and r.right == []) if not t else (r.ends[0] in r.right and r.ends[2] in r.left)
    # the tail thresholds select differently
    sizes = {t: sum(len(r.left) + len(r.right) for r in expected("shapes", "plain", t)) for t in TAILS}
    assert len(set(sizes.values())) >= 3, sizes
    forest = expected("forest", "plain", avg_tail)
    assert len(forest) == 300 and sum(len(set(r.starts)) == 3 for r in forest) >= 50
