# A/B harness for policy variants of the library on ONE GPU box (gpurun -- 'bash tools/variants_run.sh'): variants/lib_<name>.so are
# builds of csrc/ with different -D switches (variants/ is git-ignored but travels to the box); each is put in the library's place,
# runs tools/mcts_rounds.py (round trace) and the `--full` bench line, and the original library is restored.  Logs go to the directory
# given as the first argument (default variants/out).  Edit the list below.
set -e
O=${1:-variants/out}
mkdir -p "$O"
cp alphazeroforhnefatafl_amd/libtaflhip.so /tmp/lib_orig.so
for v in p0 p1 p2; do
  cp variants/lib_$v.so alphazeroforhnefatafl_amd/libtaflhip.so
  echo "== $v" >> "$O/var.log"
  python tools/mcts_rounds.py >> "$O/var.log" 2>&1
  python bench.py --full --no-cpu-baseline > "$O/var_$v.json" 2> "$O/var_$v.err"
  python -c "
import json; d=json.load(open('$O/var_$v.json')); print('$v', d['digest'][:420]); print('   executed', d['roofline']['playouts_executed'])" | tee -a "$O/var.log"
done
cp /tmp/lib_orig.so alphazeroforhnefatafl_amd/libtaflhip.so
