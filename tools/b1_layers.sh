# batch-1 per-layer profiles (ViT-S, ViT-L):  bash tools/b1_layers.sh OUT
O=${1:?usage: bash tools/b1_layers.sh OUT}
mkdir -p "$O"
timeout -k 10 300 python -u bench.py --full --batch 1 --no-b1 --no-cpu-baseline --steps 50 --layers-json "$O/b1_vits_layers.json" > "$O/b1_vits.json" 2> "$O/b1_vits.err" || exit $?
timeout -k 10 300 python -u bench.py --full --encoder vitl --batch 1 --no-b1 --no-cpu-baseline --steps 30 --layers-json "$O/b1_vitl_layers.json" > "$O/b1_vitl.json" 2> "$O/b1_vitl.err" || exit $?
