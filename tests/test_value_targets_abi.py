"""Value targets from search values (include/taflhip.h): declarations, exports, the ABI version, the two structs, the
flag values and the Python surface.  CPU only (what needs a device is in tests/test_gpu_value_targets.py)."""
import ctypes as C
import inspect
import os
import re

from alphazeroforhnefatafl_amd import _lib, abi, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"tafl_examples_value_targets": 3, "tafl_examples_gather_targets": 7, "tafl_pool_set_value_targets": 2, "tafl_pool_gather_targets": 6}


def header():
    return open(os.path.join(ROOT, "include", "taflhip.h")).read()


def test_declarations_and_exports():
    hdr = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    L = C.CDLL(_lib.LIB_PATH)
    bound = {name: args for name, _r, args in _lib.SYMBOLS}
    for name, nargs in NEW.items():
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert hasattr(L, name) and len(bound[name]) == nargs, name


def test_abi_version_stays_1():
    assert abi.ABI_VERSION == 1 and _lib.lib().tafl_abi_version() == 1
    assert re.search(r"#define\s+TAFLHIP_ABI_VERSION\s+1\b", header())


def test_the_flag_values():
    hdr = header()
    assert re.search(r"#define\s+TAFL_EXAMPLES_VALUE_TARGETS\s+0x2u", hdr) and abi.EXAMPLES_VALUE_TARGETS == 2
    assert re.search(r"#define\s+TAFL_VT_SETTLE_UNFINISHED\s+0x1u", hdr) and abi.VT_SETTLE_UNFINISHED == 1
    assert abi.EXAMPLES_SEARCH_STATS == 1


def test_the_two_structs():
    T, R = abi.TaflValueTargetsCfg, abi.TaflValueTargetsResult
    assert C.sizeof(T) == 32 == abi.EXPECTED_SIZES["tafl_value_targets_cfg"] and C.sizeof(R) == 32 == abi.EXPECTED_SIZES["tafl_value_targets_result"]
    assert [(getattr(T, f).offset, getattr(T, f).size) for f in ("lam", "flags", "_reserved")] == [(0, 8), (8, 4), (12, 20)]
    assert [(getattr(R, f).offset, getattr(R, f).size) for f in ("episodes_closed", "episodes_unfinished", "rows_with_target", "rows_settled")] == [(0, 8), (8, 8), (16, 8), (24, 8)]
    assert re.search(r"\}\s*tafl_value_targets_cfg;\s*/\*\s*32 bytes", header()) and re.search(r"\}\s*tafl_value_targets_result;\s*/\*\s*32 bytes", header())


def test_python_surface():
    assert inspect.signature(engine.BatchedGameLogic.new_examples).parameters["value_targets"].default is False
    assert inspect.signature(engine.BatchedGameLogic.new_pool).parameters["value_targets"].default is False
    assert inspect.signature(engine.Examples.value_targets).parameters["settle_unfinished"].default is False
    assert inspect.signature(engine.Examples.gather_targets).parameters["device"].default is False
    assert inspect.signature(engine.Pool.gather_targets).parameters["device"].default is False and callable(engine.Pool.set_value_targets)
