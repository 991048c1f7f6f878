"""CPU-side checks of the training-pool entry points (include/taflhip.h "training pool"): exported and bound, struct sizes as the header
documents them, and the argument errors that are decided before a device is needed."""
import ctypes as C
import os
import re

from alphazeroforhnefatafl_amd import _lib, abi
from alphazeroforhnefatafl_amd.abi import TaflPoolIngestResult, TaflPoolStats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["tafl_pool_create", "tafl_pool_destroy", "tafl_pool_clear", "tafl_pool_get_stats", "tafl_pool_ingest", "tafl_pool_trim",
       "tafl_pool_sample", "tafl_pool_gather", "tafl_pool_read"]
INVALID_ARG = -1


def test_new_symbols_are_declared_exported_and_bound():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "taflhip.h")).read(), flags=re.S)
    L = C.CDLL(_lib.LIB_PATH)
    bound = {name for name, _, _ in _lib.SYMBOLS}
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(L, name) and name in bound, name
    assert re.search(r"#define\s+TAFL_POOL_SAMPLE_SYM\s+0x1u", hdr) and abi.POOL_SAMPLE_SYM == 1
    assert _lib.lib().tafl_abi_version() == abi.ABI_VERSION == 1          # new exports only: the version stays


def test_struct_sizes():
    hdr = open(os.path.join(ROOT, "include", "taflhip.h")).read()
    for name, cls, size in (("tafl_pool_stats", TaflPoolStats, 64), ("tafl_pool_ingest_result", TaflPoolIngestResult, 32)):
        assert C.sizeof(cls) == size == abi.EXPECTED_SIZES[name]
        assert re.search(r"\}\s*%s;\s*/\*\s*%d bytes" % (name, size), hdr), name
    assert [f[0] for f in TaflPoolStats._fields_] == ["written", "live", "ingests", "oldest_generation", "skipped_open", "skipped_overflow",
                                                      "bad_slot", "device_bytes"]
    assert [f[0] for f in TaflPoolIngestResult._fields_] == ["taken", "skipped_open", "skipped_overflow", "_reserved"]


def test_argument_errors_without_a_device():
    L = _lib.lib()
    out = C.c_void_p()
    assert L.tafl_pool_create(None, 16, 8, C.byref(out)) == INVALID_ARG and not out.value
    assert L.tafl_pool_destroy(None) == 0
    assert L.tafl_pool_clear(None) == INVALID_ARG
    assert L.tafl_pool_get_stats(None, C.byref(TaflPoolStats())) == INVALID_ARG
    assert L.tafl_pool_ingest(None, None, None) == INVALID_ARG
    assert L.tafl_pool_trim(None, 1) == INVALID_ARG
    assert L.tafl_pool_sample(None, 1, 2, 0, 4, 0, None, None, None, None, None, None, 0) == INVALID_ARG
    assert L.tafl_pool_gather(None, None, None, 0, None, None, None, None, 0) == INVALID_ARG
    assert L.tafl_pool_read(None, None, 0, None, None, None, None, None) == INVALID_ARG
    assert b"null pool" in L.tafl_last_error()


def test_python_surface():
    import alphazeroforhnefatafl_amd as pkg
    from alphazeroforhnefatafl_amd import engine
    assert pkg.Pool is engine.Pool
    for m in ("ingest", "trim", "clear", "stats", "sample", "gather", "read", "close"):
        assert callable(getattr(engine.Pool, m))
    assert callable(engine.BatchedGameLogic.new_pool)
