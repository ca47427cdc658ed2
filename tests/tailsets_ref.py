"""Expected values of hga_components_overlaps and hga_components_set_scores: the two merge sequences of
tests/components_ref.py (cases A and B), each Step replayed with a tests/pyref_cluster.py Engine whose
kmer positions (`pos`) are the case's, so that Engine.overlap and Engine.accumulate answer on the lists
the step left.  The id pairs and id sets the CPU and GPU tests share are built here, with their expected
values, once per case, and the module asserts that they are not hollow:

  * per merge step at least 100 pairs whose overlap on the current lists differs from the read-level
    overlap of the same two reads (overlap_ref.read_overlaps), so an implementation that ignores the
    unions, or looks positions up in the wrong read, fails;
  * per merge step pairs with a shared KmerID that one of the two reads does not hold (position 0);
  * a survivor union of at least 0.75 K KmerIDs (K is no multiple of 32 in either case);
  * set groups whose pairwise intersections are empty, partial and full, an empty set, a set with a
    member listed twice, a set with a read without hits, a merged-away member beside its survivor.
"""
import functools

import numpy as np

import components_ref as cr
import overlap_ref


class StepRef:
    """Pairs (x, y) with overlap / shared, and sets with sizes and pair scores, on one step's lists."""

    def __init__(self, c, no, no_hit):
        st = c.steps[no]
        eng = st.engine()
        eng.pos = c.eng.pos   # positions belong to the reads: merges never change them
        self.no = no
        sv = c.all_survivors(no)
        members = [m for g in st.groups for m in g[1:]][:40]
        touched = {i for s in c.steps[:no + 1] for g in s.groups if len(g) >= 2 for i in g}
        others = [i for i in c.ids if i not in touched][:60]
        special = [no_hit] + ([c.genome_read] if hasattr(c, "genome_read") else [])
        pairs = []
        for s in st.survivors:   # survivor x survivor / member / untouched / no-hit / genome-long
            pairs += [(s, o) for o in sv + members + others + special]
        pairs += list(zip(members, members[1:]))                      # member x member
        pairs += [(a, b) for i, a in enumerate(others[:25]) for b in others[i + 1:25]]   # never merged: the plain path
        pairs += [(others[0], o) for o in special]
        pairs += [(i, i) for i in sv[:3] + members[:2] + others[:2] + special]   # x == x
        self.x = np.array([p[0] for p in pairs], np.uint32)
        self.y = np.array([p[1] for p in pairs], np.uint32)

        def overlap(a, b):
            return eng.overlap(a, b) if a in eng.comps and b in eng.comps else 0

        def shared(a, b):
            if a not in eng.comps or b not in eng.comps:
                return set()
            return set(eng.comps[a]["kmers"]) & set(eng.comps[b]["kmers"])

        self.overlap = np.array([overlap(int(a), int(b)) for a, b in pairs], np.int32)
        sh = [shared(int(a), int(b)) for a, b in pairs]
        self.shared = np.array([len(s) for s in sh], np.uint32)
        read_ov, _ = overlap_ref.read_overlaps(c.idx, self.x, self.y, c.first_id)
        self.differs = int((read_ov != self.overlap).sum())
        self.absent = sum(any(k not in eng.pos[int(a)] or k not in eng.pos[int(b)] for k in s) for (a, b), s in zip(pairs, sh))
        self.largest_union = max([len(st.kmers[s]) for s in sv], default=0)
        # the sets
        sets = []
        if sv:
            s0 = st.survivors[0]
            g0 = next(g for g in st.groups if len(g) >= 2 and g[0] == s0)
            sets += [[s0], g0[1:3], [s0, g0[1]], sv]   # a survivor, two of its members (inside it), both, all survivors
        far = self._disjoint(eng, others)
        sets += [others[:6], others[3:9], [far[0]], [far[1]],
                 [], [others[0], others[1], others[0]], [no_hit, others[2]], [no_hit]]
        if hasattr(c, "genome_read"):
            sets.append([c.genome_read])
        self.sets = [[int(i) for i in s] for s in sets]
        self.set_pairs = np.array([(a, b) for a in range(len(sets)) for b in range(a, len(sets))], np.uint32)
        unions = [set(eng.accumulate(s)) for s in self.sets]
        self.set_size = np.array([len(u) for u in unions], np.uint64)
        self.score = np.array([len(unions[a] & unions[b]) for a, b in self.set_pairs], np.uint64)

    @staticmethod
    def _disjoint(eng, ids):
        """Two ids of the list whose lists share nothing, or the pair that shares the least."""
        best = None
        for i, a in enumerate(ids):
            for b in ids[i + 1:]:
                n = len(set(eng.comps[a]["kmers"]) & set(eng.comps[b]["kmers"]))
                if best is None or n < best[0]:
                    best = (n, a, b)
                if n == 0:
                    return a, b
        return best[1], best[2]

    def kinds(self):
        """(empty, partial, full) counts over the pairs of two different non-empty sets."""
        empty = partial = full = 0
        for (a, b), s in zip(self.set_pairs.tolist(), self.score.tolist()):
            na, nb = int(self.set_size[a]), int(self.set_size[b])
            if a == b or not na or not nb:
                continue
            empty += s == 0
            full += s == min(na, nb)
            partial += 0 < s < min(na, nb)
        return empty, partial, full


class CaseRef:
    def __init__(self, c):
        self.c = c
        self.no_hit = c.first_id + int(np.flatnonzero(np.diff(c.idx["hit_ptr"]) == 0)[0])
        self.K = len(c.sdk)
        self.steps = [StepRef(c, no, self.no_hit) for no in range(len(c.steps))]
        # non-vacuity: see the module docstring
        assert self.K % 32 != 0
        assert (self.steps[0].overlap > 0).sum() >= 20 and self.steps[0].differs == 0
        for st in self.steps[1:]:
            assert st.differs >= 100, (c.name, st.no, st.differs)
            assert st.absent >= 20, (c.name, st.no, st.absent)
            assert (st.overlap == 0).any() and (st.shared > 1000).any()
        assert max(st.largest_union for st in self.steps) >= 0.75 * self.K
        for st in self.steps:
            empty, partial, full = st.kinds()
            assert partial > 0 and (full > 0 or st.no == 0), (c.name, st.no, empty, partial, full)
            assert (st.set_size == 0).sum() >= 2   # the empty set and the set of the read without hits
            assert any(len(s) != len(set(s)) for s in st.sets) and any(self.no_hit in s and len(s) > 1 for s in st.sets)
        assert sum(st.kinds()[0] for st in self.steps) > 0
        assert any(st.set_size.max() >= 0.75 * self.K for st in self.steps)


@functools.lru_cache(maxsize=None)
def case_a(hga_mod):
    return CaseRef(cr.case_a(hga_mod))


@functools.lru_cache(maxsize=None)
def case_b(hga_mod):
    return CaseRef(cr.case_b(hga_mod))
