cd $GRAFT_REPO_ROOT
O=${1:?usage: tools/_call.sh OUTDIR}
mkdir -p $O
( time python bench.py --full > $O/bench_headline.json 2> $O/bench_headline.err ) 2>&1 | grep real
python -c "
import json, sys; d=json.load(open(sys.argv[1])); a=d['also']
print(d['value'], d['ms_per_step'], d['roofline']['frac'])
print('c1', a['c1']['samples_per_s'], a['c1']['launch'], a['c1']['with_input_copy']['samples_per_s'], a['c1']['separate_optimizer_launch']['samples_per_s'])
print('c5', a['c5']['ms_per_step'])" $O/bench_headline.json
