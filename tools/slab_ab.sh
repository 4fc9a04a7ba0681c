# bench A/B: automatic choice (slab kernel on the stride-1 3x3 layers) against the ring kernel everywhere, same box
# tools/slab_ab.sh OUT_DIR   (OUT_DIR relative to the repository root; the lines of every rep -> OUT_DIR/ab.txt)
cd "$(dirname "$0")/.."; O=${1:?usage: tools/slab_ab.sh OUT_DIR}; mkdir -p "$O"
for rep in 1 2; do for c in -1 -4; do echo "== conv config $c"; AIRPOSE_CONV_CONFIG=$c timeout 300 python bench.py --full --cpu-sample 0 --parity-steps 0 --repeat-blocks 2 2>&1 | tail -1 | python -c "import sys,json; d=json.loads(sys.stdin.read()); print(d['value'], d['ms_per_step'], d['roofline']['frac'], d.get('stage_ms_per_step'))"; done; done 2>&1 | tee "$O/ab.txt"
