"""Search statistics per training row (include/taflhip.h): declarations, exports, the ABI version and the Python
surface.  CPU only (what needs a device is in tests/test_gpu_search_stats.py)."""
import ctypes as C
import inspect
import os
import re

from alphazeroforhnefatafl_amd import _lib, abi, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("tafl_examples_create_ex", "tafl_examples_read_stats", "tafl_examples_gather_stats", "tafl_pool_set_search_stats", "tafl_pool_gather_stats",
       "tafl_pool_weights_from_surprise")


def header():
    return open(os.path.join(ROOT, "include", "taflhip.h")).read()


def test_declarations_and_exports():
    hdr = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    L = C.CDLL(_lib.LIB_PATH)
    bound = {name: args for name, _r, args in _lib.SYMBOLS}
    for name in NEW:
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert hasattr(L, name) and name in bound, name
    assert len(bound["tafl_examples_create_ex"]) == 6 and len(bound["tafl_examples_read_stats"]) == 5 and len(bound["tafl_examples_gather_stats"]) == 6
    assert re.search(r"#define\s+TAFL_EXAMPLES_SEARCH_STATS\s+0x1u", hdr) and abi.EXAMPLES_SEARCH_STATS == 1


def test_abi_version_stays_1():
    assert abi.ABI_VERSION == 1 and _lib.lib().tafl_abi_version() == 1
    assert re.search(r"#define\s+TAFLHIP_ABI_VERSION\s+1\b", header())


def test_python_surface():
    assert inspect.signature(engine.BatchedGameLogic.new_examples).parameters["search_stats"].default is False
    assert inspect.signature(engine.Examples.gather_stats).parameters["device"].default is False
    assert callable(engine.Examples.read_stats)
    assert inspect.signature(engine.BatchedGameLogic.new_pool).parameters["search_stats"].default is False
    assert inspect.signature(engine.Pool.weights_from_surprise).parameters["generation"].default == 0
    assert inspect.signature(engine.Pool.gather_stats).parameters["device"].default is False and callable(engine.Pool.set_search_stats)
    for name in ("sample", "sample_weighted"):                      # (their signatures do not change)
        assert "search_stats" not in inspect.signature(getattr(engine.Pool, name)).parameters


def test_the_cfg_struct():
    T = abi.TaflPoolSurpriseWeights
    assert C.sizeof(T) == 32 and abi.EXPECTED_SIZES["tafl_pool_surprise_weights"] == 32
    assert [(getattr(T, f).offset, getattr(T, f).size) for f in ("base", "generation", "per_nat", "flags", "_reserved")] == [(0, 4), (4, 4), (8, 8), (16, 4), (20, 12)]
    assert re.search(r"\}\s*tafl_pool_surprise_weights;\s*/\*\s*32 bytes", header())


def test_the_not_offered_list_no_longer_names_priorities():
    assert "priorities computed by the library" not in header()
