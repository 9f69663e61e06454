"""The slots the search-chain diagnostics added to csrc/diag.h have names and are listed by the product library (no GPU)."""
import ptudes_lab_amd  # noqa: F401
from ptudes_lab_amd import _lib

LATER = ["search_row_key", "search_rebuild", "search_first_round", "search_survivors", "search_answer_row", "searches_timed"]
FIRST = ["search_it0_row_key", "search_it0_rebuild", "search_it0_first_round", "search_it0_survivors", "search_it0_answer_row", "searches_timed_it0"]


def test_first_iteration_laps_and_the_queue_cross_check_are_listed():
    L = _lib.lib()
    names = [L.ptl_diag_slot_name(i).decode() for i in range(L.ptl_diag_slots())]
    assert len(set(names)) == len(names)
    for nm in FIRST + ["searches_it0", "survivor_rounds_it0", "queue_kind_mismatch"]:
        assert names.count(nm) == 1, nm
    # the first iteration's set lies in the order of the later iterations' set: the search reaches it by one offset
    off = names.index(FIRST[0]) - names.index(LATER[0])
    assert off > 0 and [names.index(a) - names.index(b) for a, b in zip(FIRST, LATER)] == [off] * len(FIRST)
