"""The component merge on the CPU: the closed form of the kmer_component_index edit that the device
kernel implements (components_ref.edit_closed_form) against Engine.merge's two-pointer loop on every
KmerID of both shared cases and all their merges; the cases' non-vacuity; and the presence of the new
entry points in the header and the binding."""
import os
import re

import numpy as np
import pytest

import components_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["hga_components_merge", "hga_components_connections", "hga_components_get_sizes",
                "hga_components_fetch_index", "hga_components_fetch_kmers", "hga_components_reset"]


@pytest.mark.parametrize("make", [cr.case_a, cr.case_b], ids=["A", "B"])
def test_closed_form_equals_two_pointer_loop(make, hga_mod):
    c = make(hga_mod)
    edited = early_stop = dup_quirk = 0
    for before, after in zip(c.steps, c.steps[1:]):
        rem = cr.removal_pairs(before.kmers, after.groups)
        surv = set(after.survivors)
        for kid, (b, a) in enumerate(zip(before.kci, after.kci)):
            if kid not in rem:
                assert a == b
                continue
            got = cr.edit_closed_form(b, rem[kid]).tolist()
            assert got == a, (c.name, kid)
            edited += 1
            early_stop += any(v >= max(rem[kid]) and v not in rem[kid] for v in b)
            dup_quirk += bool(surv & set(a))
        # the unions: sorted, distinct, over the members' lists before the call
        for g in after.groups:
            if len(g) >= 2:
                assert after.kmers[g[0]] == sorted({k for i in g for k in before.kmers[i]})
                for m in g[1:]:
                    assert after.kmers[m] is before.kmers[m]
    assert edited > 1000 and early_stop > 100
    if c.name == "B":
        assert dup_quirk > 0


def test_cases_are_not_hollow(hga_mod):
    a, b = cr.case_a(hga_mod), cr.case_b(hga_mod)   # each asserts its own conditions while it is built
    assert [len(s.groups) for s in a.steps] == [0, len(a.steps[1].groups), len(a.steps[1].groups) // 2, len(a.steps[3].groups)]
    assert sorted(len(g) for g in b.steps[1].groups) == [0, 1, 2, 3, 64, 65]
    assert sorted(len(g) for g in b.steps[2].groups) == [2, 2, 151]
    # a survivor of merge 1 is a non-survivor member in merge 2, and one survives twice
    sv = b.steps[1].survivors
    assert b.steps[2].groups[0] == sv[:2] and b.steps[2].groups[1][0] == sv[2]
    # untouched ids stay untouched: their lists are the lookup's
    for i in b.rest[152:157]:
        assert b.steps[2].kmers[i] is b.steps[0].kmers[i]
    # duplicates inside a non-survivor's list give several removal pairs
    rem = cr.removal_pairs(b.steps[0].kmers, b.steps[1].groups)
    assert any(len(v) != len(set(v)) for v in rem.values())
    # an index list with a run of one read longer than one (the occurrence rank matters)
    assert any(len(l) != len(set(l)) for l in b.steps[0].kci)
    assert max(np.diff(b.idx["hit_ptr"])) > 2000


def test_entry_points_declared_and_bound(hga_mod):
    header = open(os.path.join(ROOT, "include", "hga.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"hga_status\s+%s\s*\(" % name, header), name
        assert name in hga_mod.HGA_SYMBOLS, name
    assert "hga_components_sizes" in header
    for meth in ("components_merge", "components_connections", "components_sizes", "components_index",
                 "components_kmers", "components_reset"):
        assert callable(getattr(hga_mod.Ctx, meth, None)), meth
    assert [f for f, _ in hga_mod.ComponentsSizes._fields_] == ["index_entries", "survivors", "survivor_kmers", "merges"]
