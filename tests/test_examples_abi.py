"""CPU-side checks of the training-example entry points (include/taflhip.h "self-play that records training examples"): exported and
bound, struct sizes as documented, and the argument errors that are decided before a device is needed."""
import ctypes as C
import os
import re

from alphazeroforhnefatafl_amd import _lib, abi
from alphazeroforhnefatafl_amd.abi import TaflExamplesStats, TaflMctsParams, TaflSelfplayOpts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["tafl_examples_create", "tafl_examples_destroy", "tafl_examples_clear", "tafl_examples_counts", "tafl_examples_get_stats",
       "tafl_selfplay_record", "tafl_examples_finalize", "tafl_examples_read", "tafl_examples_gather"]
INVALID_ARG, UNSUPPORTED = -1, -5


def test_new_symbols_are_declared_exported_and_bound():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "taflhip.h")).read(), flags=re.S)
    L = C.CDLL(_lib.LIB_PATH)
    bound = {name for name, _, _ in _lib.SYMBOLS}
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(L, name) and name in bound, name
    assert _lib.lib().tafl_abi_version() == abi.ABI_VERSION == 1          # new exports only: the version stays


def test_struct_sizes():
    hdr = open(os.path.join(ROOT, "include", "taflhip.h")).read()
    for name, cls in (("tafl_selfplay_opts", TaflSelfplayOpts), ("tafl_examples_stats", TaflExamplesStats)):
        assert C.sizeof(cls) == 32 == abi.EXPECTED_SIZES[name]
        assert re.search(r"\}\s*%s;\s*/\*\s*32 bytes" % name, hdr), name
    assert [f[0] for f in TaflSelfplayOpts._fields_] == ["sample_seed", "temp_moves", "move_base", "flags", "_reserved"]
    assert TaflSelfplayOpts.temp_moves.offset == 8 and TaflSelfplayOpts.flags.offset == 16


def test_argument_errors_without_a_device():
    L = _lib.lib()
    out = C.c_void_p()
    assert L.tafl_examples_create(None, 4, 4, 4, C.byref(out)) == INVALID_ARG and not out.value
    assert L.tafl_examples_destroy(None) == 0
    assert L.tafl_examples_clear(None) == INVALID_ARG
    assert L.tafl_examples_counts(None, None, None) == INVALID_ARG
    assert L.tafl_examples_get_stats(None, C.byref(TaflExamplesStats())) == INVALID_ARG
    assert L.tafl_examples_finalize(None, None) == INVALID_ARG
    assert L.tafl_examples_read(None, None, 0, None, None, None, None, None, None) == INVALID_ARG
    assert L.tafl_examples_gather(None, None, None, 0, None, None, None, None, None, 0) == INVALID_ARG
    assert b"null examples object" in L.tafl_last_error()
    p, o = TaflMctsParams(8, 64, 1.0, 1, 0, 0), TaflSelfplayOpts(1, 0, 0, 0)
    assert L.tafl_selfplay_record(None, C.byref(p), C.byref(o), 2, 0, None, None) == INVALID_ARG           # no batch
    assert L.tafl_selfplay_record(None, None, C.byref(o), 2, 0, None, None) == INVALID_ARG
    assert L.tafl_selfplay_record(None, C.byref(p), None, 2, 0, None, None) == INVALID_ARG
    assert L.tafl_selfplay_record(None, C.byref(p), C.byref(o), 0, 0, None, None) == INVALID_ARG
    # the parameters are judged before the batch is looked at: what tafl_selfplay_run rejects, and the reserved words of the options
    keep = TaflMctsParams(8, 64, 1.0, 1, 0, abi.MCTS_FLAG_KEEP_TREE)
    assert L.tafl_selfplay_record(None, C.byref(keep), C.byref(o), 2, 0, None, None) == UNSUPPORTED
    assert b"KEEP_TREE" in L.tafl_last_error()
    assert L.tafl_selfplay_record(None, C.byref(p), C.byref(TaflSelfplayOpts(1, 0, 0, 1)), 2, 0, None, None) == UNSUPPORTED
    res = TaflSelfplayOpts(1, 0, 0, 0)
    res._reserved[2] = 1
    assert L.tafl_selfplay_record(None, C.byref(p), C.byref(res), 2, 0, None, None) == UNSUPPORTED
    wide = TaflMctsParams(70000, 64, 1.0, 1, 0, 0)
    assert L.tafl_selfplay_record(None, C.byref(wide), C.byref(o), 2, 0, None, None) == INVALID_ARG
    big = TaflMctsParams(60000, 64, 1.0, 1, 0xFFFF0000, 0)
    assert L.tafl_selfplay_record(None, C.byref(big), C.byref(o), 8, 0, None, None) == INVALID_ARG


def test_python_surface():
    import alphazeroforhnefatafl_amd as pkg
    from alphazeroforhnefatafl_amd import engine, selfplay
    assert pkg.play_episodes is selfplay.play_episodes and pkg.Examples is engine.Examples
    for m in ("clear", "counts", "stats", "finalize", "read", "gather", "close"):
        assert callable(getattr(engine.Examples, m))
    assert callable(engine.BatchedGameLogic.new_examples) and callable(engine.GameBatch.selfplay_record)
