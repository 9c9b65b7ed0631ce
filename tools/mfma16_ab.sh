# A/B of the MFMA shape of the stride-1 bf16 3x3 convs inside ONE library (DH_CONV_MFMA16=0 / 1, same box): headline, phase stamps with the
# in-kernel clock, per-layer kernel times, and bank conflicts from a counters-only pass.  Tooling only.  usage: bash tools/mfma16_ab.sh [passes]
set -e -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd); O=$(mktemp -d); cd $R
for rep in $(seq 1 ${1:-3}); do
  for k in 0 1; do
    DH_CONV_MFMA16=$k timeout -k 10 300 python3 bench.py 2>/dev/null | python3 -c "import json,sys; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print('DH_CONV_MFMA16=$k', round(d['value']), 'patches/s')"
  done
done
for k in 0 1; do
  echo "== DH_CONV_MFMA16=$k"
  DH_CONV_MFMA16=$k timeout -k 10 300 python3 tools/conv_stamps.py 3968 2>/dev/null | { grep -v "^stem" || true; }
  rm -rf $O/m16_tr_$k $O/m16_pmc_$k
  DH_CONV_MFMA16=$k timeout -k 10 600 rocprofv3 --output-format csv --kernel-trace --stats -d $O/m16_tr_$k -o t -- python3 bench.py > /dev/null 2> $O/m16_tr_$k.err
  python3 tools/trace_summary.py $O/m16_tr_$k 3968
  DH_CONV_MFMA16=$k timeout -k 10 300 rocprofv3 --output-format csv --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE -d $O/m16_pmc_$k -o c -- python3 tools/fwd_once.py 3968 2 > $O/m16_pmc_$k.log 2>&1
  python3 tools/pmc_layers.py $O/m16_pmc_$k
  rm -rf $O/m16_tr_$k $O/m16_pmc_$k
done
rm -rf $O
