# the whole -m gpu suite + the bench line with every figure (--full), from the repository root; results under OUT_DIR
O=${1:?usage: bash tools/gpu/full.sh OUT_DIR}
mkdir -p "$O" && O=$(cd "$O" && pwd) && cd "$(dirname "$0")/../.." || exit 1
timeout 3000 python -m pytest tests -m gpu -x -q 2>&1 | tail -15 | tee "$O/tests.txt"
timeout 600 python bench.py --full --steps 20 --warmup 5 > "$O/bench.json" 2> "$O/bench.err"; tail -c 300 "$O/bench.err"; cut -c1-1500 "$O/bench.json"
python3 -c "
import json, sys; d=json.load(open(sys.argv[1])); print(d['cpu_baseline']); print(d['check'])" "$O/bench.json"
