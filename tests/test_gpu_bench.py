"""bench.py on a real MI355X: a plain run times exactly --steps steps, carries none of the --full objects, and
--dump-outputs writes what its last timed step computed, which must equal the oracle on the same games.  `pytest -m gpu`."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from alphazeroforhnefatafl_amd import abi
from alphazeroforhnefatafl_amd.abi import TaflMctsParams
from oracle import oracle as orc
from tests import parity_util as pu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_and_dumped_outputs(tmp_path):
    games, sims, cap, seed = 2048, 64, 512, 2                     # bench.py defaults except the batch size
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--games", str(games), "--dump-outputs", str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 3 and line["ms_per_step"] > 0
    assert line["metric"] == "mcts_sims_per_sec" and line["unit"] == "sims/s" and line["higher_is_better"] is True
    assert "variants" not in line and "cpu_baseline" not in line

    d = {f[:-4]: np.load(tmp_path / f) for f in sorted(os.listdir(tmp_path))}
    assert set(d) == {"root_children_count", "root_best_action", "root_best_visits", "sample_games",
                      "sample_root_action", "sample_root_visits", "sample_root_q"}
    assert all(a.dtype in (np.float32, np.float64) for a in d.values())
    assert sum(a.nbytes for a in d.values()) <= 64 << 20
    assert d["root_children_count"].shape == (games,) and d["sample_root_q"].shape == (games, sims)
    sample = d["sample_games"].astype(np.int64)
    assert (np.diff(sample) > 0).all()

    lg = orc.GameLogic(abi.rules.COPENHAGEN, 11)
    p = TaflMctsParams(sims, cap, 1.0, seed, 0, 0)
    for i in (0, len(sample) // 2, len(sample) - 1):
        g = int(sample[i])
        one = pu.start_states(orc, abi.boards.COPENHAGEN, abi.rules.COPENHAGEN.starting_side, 128, 1)
        ok, on, _ = orc.batch_mcts(lg, one, 1, 128, p, g)
        n = int(on[0])
        assert d["root_children_count"][g] == n
        assert [int(x) for x in d["sample_root_action"][i, :n]] == [ok[j].action for j in range(n)]
        assert [int(x) for x in d["sample_root_visits"][i, :n]] == [ok[j].visits for j in range(n)]
        assert [float(x).hex() for x in d["sample_root_q"][i, :n]] == [float(ok[j].q).hex() for j in range(n)]
        assert (d["sample_root_action"][i, n:] == -1).all() and (d["sample_root_visits"][i, n:] == 0).all()
        best = max(range(n), key=lambda j: (ok[j].visits, -j))
        assert d["root_best_action"][g] == ok[best].action and d["root_best_visits"][g] == ok[best].visits
