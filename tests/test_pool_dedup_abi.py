"""De-duplication of the training pool (include/taflhip.h): declarations, exports, the ABI version, the structs and
the Python surface.  CPU only (what needs a device is in tests/test_gpu_pool_dedup.py)."""
import ctypes as C
import inspect
import os
import re

from alphazeroforhnefatafl_amd import _lib, abi, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"tafl_pool_dedup": 3, "tafl_pool_gather_dedup": 7, "tafl_pool_weights_from_dedup": 2}


def header():
    return open(os.path.join(ROOT, "include", "taflhip.h")).read()


def test_declarations_and_exports():
    hdr = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    L = C.CDLL(_lib.LIB_PATH)
    bound = {name: args for name, _r, args in _lib.SYMBOLS}
    for name, nargs in NEW.items():
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert hasattr(L, name) and len(bound[name]) == nargs, name
    for name, value in (("TAFL_POOL_DEDUP_SYMMETRIES", 1), ("TAFL_POOL_DEDUP_DIVIDE", 1), ("TAFL_POOL_DEDUP_REPRESENTATIVES", 2)):
        assert re.search(r"#define\s+%s\s+0x%xu" % (name, value), hdr), name
    assert (abi.POOL_DEDUP_SYMMETRIES, abi.POOL_DEDUP_DIVIDE, abi.POOL_DEDUP_REPRESENTATIVES) == (1, 1, 2)


def test_abi_version_stays_1():
    assert abi.ABI_VERSION == 1 and _lib.lib().tafl_abi_version() == 1
    assert re.search(r"#define\s+TAFLHIP_ABI_VERSION\s+1\b", header())


def _layout(T, names):
    return [(getattr(T, f).offset, getattr(T, f).size) for f in names]


def test_the_structs():
    assert _layout(abi.TaflPoolDedupCfg, ("flags", "key_bits", "_reserved")) == [(0, 4), (4, 4), (8, 24)]
    assert _layout(abi.TaflPoolDedupResult, ("live", "distinct", "largest", "collisions", "device_bytes", "_reserved")) == [(0, 8), (8, 8), (16, 8), (24, 8), (32, 8), (40, 24)]
    assert _layout(abi.TaflPoolDedupWeights, ("scale", "flags", "_reserved")) == [(0, 4), (4, 4), (8, 24)]
    for name, T, size in (("tafl_pool_dedup_cfg", abi.TaflPoolDedupCfg, 32), ("tafl_pool_dedup_result", abi.TaflPoolDedupResult, 64),
                          ("tafl_pool_dedup_weights", abi.TaflPoolDedupWeights, 32)):
        assert C.sizeof(T) == size == abi.EXPECTED_SIZES[name]
        assert re.search(r"\}\s*%s;\s*/\*\s*%d bytes" % (name, size), header()), name


def test_python_surface():
    p = inspect.signature(engine.Pool.dedup).parameters
    assert p["symmetries"].default is False and p["key_bits"].default == 64
    assert inspect.signature(engine.Pool.gather_dedup).parameters["device"].default is False
    p = inspect.signature(engine.Pool.weights_from_dedup).parameters
    assert list(p)[1] == "scale" and p["divide"].default is False and p["representatives"].default is False
    assert callable(engine.Pool.free_dedup)


def test_the_not_offered_list_no_longer_names_deduplication():
    assert "de-duplication of positions" not in header() and "de-duplication at ingest" in header()
