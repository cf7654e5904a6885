"""The expectation table of tests/ordering_util.py against the rules of DESIGN.md 4.9, written out here a second time in the
words of the section: every ordered pair of operations has exactly one entry, and the entries follow the rules."""
import itertools

import ordering_util as ou

FRAME_LIKE = {"frame", "aov"}
READERS = {"query", "shade", "radiance"}
EDITS = {"update", "replace", "pose", "pose_skin"}


def _waits(a, b):
    """Does B wait for A?  The sentences of the issue and of 4.9, one per line."""
    if b in FRAME_LIKE:
        return a in FRAME_LIKE or a in EDITS                 # frame and AOV wait for: frame, AOV, edit
    if b in READERS:
        return a in EDITS or a in READERS                    # readers wait for: edit, every reader family
    if b in EDITS:
        return a in FRAME_LIKE or a in READERS or a in EDITS  # edits wait for: frame, every reader, AOV, edit
    if b == "filter":
        return a == "filter"                                 # filter waits only for filter
    if b == "accumulate":
        return a == "accumulate"                             # accumulate waits only for accumulate
    raise AssertionError(b)


def test_the_operations_are_the_issues():
    assert set(ou.OPS) == FRAME_LIKE | READERS | EDITS | {"filter", "accumulate"}
    assert len(ou.OPS) == len(set(ou.OPS)) == 11
    assert set(ou.KIND) == set(ou.OPS)


def test_every_ordered_pair_has_exactly_one_entry():
    want = set(itertools.product(ou.OPS, repeat=2))
    assert set(ou.TABLE) == want and len(ou.TABLE) == len(ou.OPS) ** 2


def test_the_entries_follow_the_rules():
    for (a, b), exp in ou.TABLE.items():
        assert exp.waits == _waits(a, b), (a, b)
        assert exp.how == ("data" if a in EDITS and b in EDITS else "gate"), (a, b)
    # nothing waits for a filter or an accumulate call but its own family
    for a in ("filter", "accumulate"):
        assert [b for b in ou.OPS if ou.TABLE[(a, b)].waits] == [a]


def test_the_holder_of_an_edit_has_no_edge_to_b():
    for b in ou.OPS:
        if b in EDITS:
            continue
        z = ou.holder_for(b)
        assert not ou.TABLE[(z, b)].waits                    # B is held by the edit alone
        assert all(ou.TABLE[(z, e)].waits for e in EDITS)    # and the edit by Z


def test_what_the_contexts_run():
    main = [op for op in ou.OPS if op != "pose_skin"]
    # (b) runs the whole matrix of its operations, but for a pose right after the update or replace that dropped its table
    assert set(ou.CONTEXT_PAIRS["b"]) == set(itertools.product(main, repeat=2)) - {("update", "pose"), ("replace", "pose")}
    assert {a for a, _ in ou.CONTEXT_PAIRS["a"]} == {"frame", "aov", "update", "pose"}
    assert all({b for x, b in ou.CONTEXT_PAIRS["a"] if x == a} >= set(main) - {"pose"} for a in ("frame", "aov", "update", "pose"))
    assert len(ou.CONTEXT_PAIRS["c"]) == 6 and ("frame", "frame") in ou.CONTEXT_PAIRS["c"]
    assert {b for a, b in ou.CONTEXT_PAIRS["skin"] if a == "pose_skin"} == {"frame", "query", "aov", "filter"}
    ids = ou.all_case_ids()
    assert len(ids) == len(set(ids)) == sum(len(v) for v in ou.CONTEXT_PAIRS.values())
    # every cell of the table between the main operations is run somewhere, with the two exceptions above
    assert all(ctx_pair in ou.TABLE for pairs in ou.CONTEXT_PAIRS.values() for ctx_pair in pairs)
