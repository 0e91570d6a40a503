# A/B of env settings on one bench config: bash tools/ab_cfg.sh cfg5 "<env,env> <env> ..." [steps]
set -e
OUT=${OUT:-ab_out}; mkdir -p $OUT  # results directory (override with OUT=...)
i=0
for cfg in $2; do
  i=$((i+1))
  env $(echo $cfg | tr ',' ' ') timeout -k 10 300 python bench.py --config $1 --steps ${3:-20} --warmup 3 --full --no-cpu-baseline --no-ifft-stage --no-beyond-cache > $OUT/abc_$i.json 2> $OUT/abc_$i.err
  echo "$cfg $(python -c "import json;d=json.load(open('$OUT/abc_$i.json'));print(d['value'],d['kernels_us'])")"
done
