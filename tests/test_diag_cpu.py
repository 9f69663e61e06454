"""The diagnostic slots' host surface on the product library (no GPU): the slot list of csrc/diag.h as the library reports it."""
import ptudes_lab_amd  # noqa: F401
from ptudes_lab_amd import _lib, core

from test_map_score_cpu import _declared, _exported

NEW = {"ptl_diag_slots", "ptl_diag_slot_name", "ptl_icp_diag"}


def test_diag_surface_of_the_product_library():
    declared, exported = _declared(), _exported(_lib.LIB_PATH)
    assert NEW <= declared and NEW <= exported
    L = _lib.lib()
    for name in NEW:
        assert getattr(L, name).argtypes == _lib.PROTOTYPES[name][1]
    assert L.ptl_abi_version() == 6 == _lib.ABI_VERSION  # new entry points change no struct or prototype
    n = L.ptl_diag_slots()
    assert n > 0
    names = [L.ptl_diag_slot_name(i) for i in range(n)]
    assert all(names) and len(set(names)) == n
    assert L.ptl_diag_slot_name(-1) is None and L.ptl_diag_slot_name(n) is None
    assert core.build_info()["diagnostics"] == 0  # the product build carries no diagnostic flavour
    # every value the tools read by name exists
    want = {"searches", "survivor_rounds", "rows_rebuilt", "bound_candidate", "bound_box", "bound_ratio_4", "point_loop_first", "point_loop_others",
            "phase_a_chunks", "search_passes", "searches_timed", "tails", "miss_same_neighbour", "misses_at_iteration_23", "sq_prune", "k1_count",
            "map_site_3", "map_first_b"}
    assert want <= {nm.decode() for nm in names}
