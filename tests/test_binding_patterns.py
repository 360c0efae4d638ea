"""The ctypes signatures of the solver family are declared once (dsurftomo_amd.engine.declare_solvers): the engine's own handle of the
library (load_library) and a bare handle bound by invert.bind must carry the same ones.  No GPU: nothing here calls into the library."""
import ctypes as C
import os
import re

from dsurftomo_amd import engine, invert

FAMILY = ("dsa_lsmr", "dsa_lsmr_batch", "dsa_lsmr_resolution", "dsa_lsmr_tradeoff", "dsa_lsmr_crossval", "dsa_lsmr_voronoi", "dsa_lsmr_dropin",
          "dsa_iteration_system", "dsa_iteration_system_device", "dsa_model_update", "dsa_error_string")


def test_bare_and_engine_handles_carry_the_same_signatures():
    from dsurftomo_amd import build
    bare = invert.bind(C.CDLL(build.build()))
    own = engine.load_library()
    assert invert.bind(own) is own
    assert bare is not own
    for name in FAMILY:
        a, b = getattr(bare, name), getattr(own, name)
        assert a.argtypes == b.argtypes, name
        assert a.restype is b.restype, name
        if name != "dsa_lsmr_dropin":                                # (Fortran-style: every argument by reference, passed with byref)
            assert a.argtypes, name
    # every dsa_lsmr* the header exports is in FAMILY
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "dsurftomo_amd.h")).read()
    assert set(re.findall(r"\b(dsa_lsmr\w*)\s*\(", header)) <= set(FAMILY)
    assert bare.dsa_error_string.restype is C.c_char_p and bare.dsa_lsmr_batch.argtypes[4:9] == [C.c_float] * 4 + [C.c_int]
