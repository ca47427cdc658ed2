"""Expected values of hga_components_*: the two merge sequences the CPU and GPU component tests share,
replayed once with tests/pyref_cluster.py's Engine (merge, get_connections), and the closed form of the
kmer_component_index edit in numpy.

Case A (realistic): overlap_ref.nanosim_case with ReadIDs from 1000; short index lists, no read with a
duplicate KmerID; three merges shaped like run_clustering's (scaffold union-find, a merge of survivors,
enrichment).  Case B (pileup): a 4 kb genome with a 200-base block twice in a row under 330 long reads,
so index lists run to several hundred entries, most reads hold a KmerID twice, and the edit's early stop
and the survivor-listed-once quirk both occur; two merges with groups of 0, 1, 2, 3, 64 and 65 members.
"""
import functools

import numpy as np

import oracle
import overlap_ref
import pyref_cluster as pc


def edit_closed_form(lst, rem):
    """The reference's two-pointer edit of one index list (ascending, duplicates allowed) against a
    non-empty removal multiset: the j-th occurrence (from 0) of value c stays exactly when c < max(rem)
    and j >= the multiplicity of c in rem."""
    lst, rem = np.asarray(lst, np.int64), np.sort(np.asarray(rem, np.int64))
    j = np.arange(len(lst)) - np.searchsorted(lst, lst, "left")
    mult = np.searchsorted(rem, lst, "right") - np.searchsorted(rem, lst, "left")
    return lst[(lst < rem[-1]) & (j >= mult)]


def removal_pairs(kmers, groups):
    """{kid: [ids]} of one merge call from the lists before it: per entry of a non-survivor member's
    list, per distinct KmerID of the group's union for the survivor."""
    out = {}
    for g in groups:
        if len(g) < 2:
            continue
        union = sorted({k for i in g for k in kmers[i]})
        for k in union:
            out.setdefault(k, []).append(g[0])
        for m in g[1:]:
            for k in kmers[m]:
                out.setdefault(k, []).append(m)
    return out


class Step:
    """The state after one merge call: groups as passed, kci (list per KmerID), kmers {id: list}."""

    def __init__(self, groups, eng):
        self.groups = [list(map(int, g)) for g in groups]
        self.kci = [list(l) for l in eng.kci]
        self.kmers = {i: c["kmers"] for i, c in eng.comps.items()}   # merge replaces lists, never edits them
        self.survivors = [g[0] for g in self.groups if len(g) >= 2]

    def engine(self):
        e = object.__new__(pc.Engine)
        e.debug = False
        e.kci = self.kci
        e.comps = {i: {"kmers": k} for i, k in self.kmers.items()}
        return e

    def connections(self, pivots, min_score):
        return [(x, y, s) for x, y, s, _ in self.engine().get_connections([int(p) for p in pivots], min_score)]

    def csr(self):
        ptr = np.concatenate([[0], np.cumsum([len(l) for l in self.kci])]).astype(np.uint64)
        ids = np.array([v for l in self.kci for v in l], np.uint32)
        return ptr, ids


class Case:
    def __init__(self, name, bases, offsets, k, sdk, idx, first_id):
        self.name, self.bases, self.offsets, self.k, self.sdk, self.idx, self.first_id = \
            name, bases, offsets, k, sdk, idx, first_id
        n = len(offsets) - 1
        self.n = n
        self.eng = pc.Engine(idx, np.diff(offsets), np.zeros(n, np.int32), 0, False, {}, first_id)
        self.ids = sorted(self.eng.comps)
        self.steps = [Step([], self.eng)]   # steps[0]: the lookup's state

    def merge(self, groups):
        self.eng.merge([list(g) for g in groups])
        self.steps.append(Step(groups, self.eng))
        return self.steps[-1]

    def all_survivors(self, upto):
        s = set()
        for st in self.steps[:upto + 1]:
            s |= set(st.survivors)
        return sorted(s)


def edit_stats(before, after, groups):
    """Counts over the KmerIDs of one merge: untouched, changed, truncating (a read outside the call's
    groups is dropped by the early stop), entries left, lists still naming a survivor, empty lists."""
    members = {i for g in groups if len(g) >= 2 for i in g}
    surv = {g[0] for g in groups if len(g) >= 2}
    st = dict(untouched=0, changed=0, truncating=0, entries=0, list_survivor=0, empty=0, longest=0, above256=0)
    for b, a in zip(before, after):
        st["untouched" if a == b else "changed"] += 1
        if set(b) - set(a) - members:
            st["truncating"] += 1
        st["entries"] += len(a)
        st["list_survivor"] += bool(surv & set(a))
        st["empty"] += not a
        st["longest"] = max(st["longest"], len(a))
        st["above256"] += len(a) > 256
    return st


@functools.lru_cache(maxsize=None)
def case_a(hga_mod):
    first_id = 1000
    bases, offsets, k, sdk, idx = overlap_ref.nanosim_case(hga_mod, first_id)
    c = Case("A", bases, np.asarray(offsets, np.uint64), k, sdk, idx, first_id)
    conns = c.eng.get_connections(c.ids, 1)
    g1 = [comp for comp, _ in pc.union_find(conns[:int(len(conns) * 0.3)], set(), 3, 40)]
    c.merge(g1)
    sv = [g[0] for g in g1]
    c.merge([sv[i:i + 2] for i in range(0, len(sv) - 1, 2)])
    sv2 = c.steps[2].survivors
    g3 = [comp for comp, _ in pc.union_find(c.eng.get_connections(sv2, 4), set(sv2), 2, -1)]
    c.merge(g3)
    # non-vacuity: see the module docstring
    s1 = edit_stats(c.steps[0].kci, c.steps[1].kci, g1)
    assert len(conns) > 10_000 and len(g1) >= 5 and max(map(len, g1)) == 40 and min(map(len, g1)) >= 3
    assert s1["untouched"] > 0 and s1["changed"] > 1000 and s1["truncating"] > 100 and 0 < s1["entries"] < len(idx["kci_read"])
    assert len(c.steps[2].survivors) >= 3 and len(g3) >= 2 and max(map(len, g3)) > 40
    assert 0 < sum(map(len, c.steps[3].kci)) < s1["entries"]
    return c


@functools.lru_cache(maxsize=None)
def case_b(hga_mod):
    k, first_id = 15, 7
    g = hga_mod.gen_genome(4000, 31)
    g = g[:2000] + g[1800:2000] + g[2000:]
    codes, _ = oracle.kmer_windows(g, k)
    sdk = np.unique(codes)[::2]
    rng = np.random.default_rng(3)
    reads = []
    for _ in range(330):
        ln = int(rng.integers(1500, 4201))
        s = int(rng.integers(0, len(g) - ln + 1))
        reads.append(g[s:s + ln])
    reads += [b"A" * 100, g[:k], g]
    bases = b"".join(reads)
    offsets = np.cumsum([0] + [len(r) for r in reads]).astype(np.uint64)
    idx = oracle.construct_indices(bases, offsets, k, sdk, first_id)
    c = Case("B", bases, offsets, k, sdk, idx, first_id)
    c.no_hit, c.genome_read = first_id + 330, first_id + 332
    perm = [int(v) for v in rng.permutation(np.arange(first_id, first_id + 330))]
    g1, at = [[perm[134]]], 0
    for size in (2, 3, 64, 65):
        g1.append(perm[at:at + size])
        at += size
    g1.append([])
    c.merge(g1)
    sv = c.steps[1].survivors
    used = {i for grp in g1 if len(grp) >= 2 for i in grp}   # the one-member group's id stays outside
    rest = [i for i in range(first_id, first_id + 330) if i not in used]
    c.rest = rest
    c.merge([sv[:2], [sv[2]] + rest[:150], rest[150:152]])
    lens = np.diff(idx["kci_ptr"])
    hp, sk = idx["hit_ptr"], idx["sorted_kid"]
    dup_reads = sum(len(set(sk[hp[i]:hp[i + 1]].tolist())) < hp[i + 1] - hp[i] for i in range(c.n))
    s1 = edit_stats(c.steps[0].kci, c.steps[1].kci, g1)
    s2 = edit_stats(c.steps[1].kci, c.steps[2].kci, c.steps[2].groups)
    assert c.no_hit not in c.eng.comps and len(c.eng.comps[c.genome_read]["kmers"]) > len(sdk)
    assert (lens > 256).sum() > 100 and ((lens > 64) & (lens <= 256)).sum() > 100 and (lens <= 64).sum() > 10
    assert dup_reads > 100
    assert s1["truncating"] > 100 and s1["list_survivor"] > 0 and s1["above256"] > 0 and s1["longest"] > 256
    assert 0 < s1["entries"] < len(idx["kci_read"]) and 0 < s2["entries"] < s1["entries"] and s2["empty"] > 0
    return c


def stats(c):
    """Figures for eyeballing a case against the numbers its description gives."""
    out = []
    for i in range(1, len(c.steps)):
        st = edit_stats(c.steps[i - 1].kci, c.steps[i].kci, c.steps[i].groups)
        out.append((sorted(len(g) for g in c.steps[i].groups), st))
    return out
