"""The model-export entry points on a CPU-only machine: declared in the header with their `what` codes,
exported by the binding, and refused by the host stand-in before anything is done (it has no device
views, as for the tensor export)."""
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "pairwise-perturbation_amd"))
import ppals  # noqa: E402

HEADER = open(os.path.join(ROOT, "include", "ppals.h")).read()


def test_header_declares_both_exports_and_the_what_codes():
    for fn in ("ppals_cp_export_model_device", "ppals_tucker_export_model_device"):
        assert re.search(r"\bint\s+" + fn + r"\s*\(", HEADER), fn
        assert fn in ppals.EXPORTS
    assert int(re.search(r"#define PPALS_MODEL\s+(\d+)", HEADER).group(1)) == ppals.MODEL == 0
    assert int(re.search(r"#define PPALS_RESIDUAL\s+(\d+)", HEADER).group(1)) == ppals.RESIDUAL == 1


def test_sessions_offer_the_torch_helpers():
    for cls in (ppals.CP, ppals.Tucker):
        for m in ("export_model_device", "export_model_torch", "model_to_torch"):
            assert callable(getattr(cls, m, None)), (cls.__name__, m)
