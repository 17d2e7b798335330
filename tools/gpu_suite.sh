# The whole GPU test suite + one full bench line on the GPU box:  bash tools/gpu_suite.sh OUT_DIR  -> OUT_DIR/tests.txt, OUT_DIR/bench.json
out=${1:?usage: tools/gpu_suite.sh OUT_DIR}
mkdir -p "$out"
timeout 2400 python -m pytest tests -q -m gpu -x 2>&1 | tail -30 > "$out/tests.txt"
python bench.py --full --no-dp-projection --no-cpu-baseline 2>/dev/null | tail -1 > "$out/bench.json"
