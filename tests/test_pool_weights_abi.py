"""CPU-side checks of the weighted-sampling entry points of the training pool (include/taflhip.h tafl_pool_set_weighting / _set_weights /
_get_weights / _sample_weighted / _weight_stats): exported and bound, struct sizes as the header documents them, the argument errors that
are decided before a device is needed, and the Python surface."""
import ctypes as C
import inspect
import os
import re

from alphazeroforhnefatafl_amd import _lib, abi
from alphazeroforhnefatafl_amd.abi import TaflPoolWeightCounters, TaflPoolWeights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["tafl_pool_set_weighting", "tafl_pool_set_weights", "tafl_pool_get_weights", "tafl_pool_sample_weighted", "tafl_pool_weight_stats"]
INVALID_ARG = -1


def test_new_symbols_are_declared_exported_and_bound():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "taflhip.h")).read(), flags=re.S)
    L = C.CDLL(_lib.LIB_PATH)
    bound = {name: args for name, _, args in _lib.SYMBOLS}
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(L, name) and name in bound, name
    assert len(bound["tafl_pool_sample_weighted"]) == 15 and len(bound["tafl_pool_set_weights"]) == 5 and len(bound["tafl_pool_get_weights"]) == 5
    assert _lib.lib().tafl_abi_version() == abi.ABI_VERSION == 1          # new exports only: the version stays


def test_struct_sizes():
    hdr = open(os.path.join(ROOT, "include", "taflhip.h")).read()
    for name, cls, size in (("tafl_pool_weights", TaflPoolWeights, 32), ("tafl_pool_weight_counters", TaflPoolWeightCounters, 64)):
        assert C.sizeof(cls) == size == abi.EXPECTED_SIZES[name]
        assert re.search(r"\}\s*%s;\s*/\*\s*%d bytes" % (name, size), hdr), name
    assert [f[0] for f in TaflPoolWeights._fields_] == ["ingest_weight", "flags", "_reserved"]
    assert [f[0] for f in TaflPoolWeightCounters._fields_] == ["enabled", "ingest_weight", "total_weight", "positive", "bad_slot", "rebuilds",
                                                               "device_bytes", "_reserved"]
    assert TaflPoolWeights.flags.offset == 4 and TaflPoolWeightCounters.device_bytes.offset == 48


def test_header_no_longer_lists_weighted_sampling_as_missing():
    hdr = open(os.path.join(ROOT, "include", "taflhip.h")).read()
    missing = hdr[hdr.index("Not offered: saving and loading a pool"):]
    assert "weighted or prioritised sampling" not in missing[:missing.index("*/")]
    assert "0x504F4F4C57445257" in hdr


def test_argument_errors_without_a_device():
    L = _lib.lib()
    w = TaflPoolWeights(ingest_weight=1)
    assert L.tafl_pool_set_weighting(None, C.byref(w)) == INVALID_ARG
    assert L.tafl_pool_set_weighting(None, None) == INVALID_ARG
    assert L.tafl_pool_set_weights(None, None, None, 0, 0) == INVALID_ARG
    assert L.tafl_pool_get_weights(None, None, 0, None, 0) == INVALID_ARG
    assert L.tafl_pool_sample_weighted(None, 1, 2, 0, 4, 0, None, None, None, None, None, None, None, None, 0) == INVALID_ARG
    assert L.tafl_pool_weight_stats(None, C.byref(TaflPoolWeightCounters())) == INVALID_ARG
    assert b"null pool" in L.tafl_last_error()


def test_python_surface():
    from alphazeroforhnefatafl_amd import engine
    for m in ("set_weighting", "set_weights", "weights", "sample_weighted", "weight_stats"):
        assert callable(getattr(engine.Pool, m))
    assert list(inspect.signature(engine.Pool.sample_weighted).parameters) == ["self", "count", "seed", "step", "row_base", "symmetries", "device"]
    assert list(inspect.signature(engine.Pool.set_weights).parameters) == ["self", "slots", "weights", "device"]
    # Pool.sample keeps its signature
    assert list(inspect.signature(engine.Pool.sample).parameters) == ["self", "count", "seed", "step", "row_base", "symmetries", "device"]
