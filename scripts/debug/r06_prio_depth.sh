mkdir -p bench_out/r06r
B=$PWD/deeppointmap_amd/csrc/build
run() { tag=$1; lib=$2; shift 2; env $lib python bench.py --full --steps 60 --warmup 10 --no-extras --cpu-frames 0 --allow-knobs "$@" > bench_out/r06r/$tag.json 2> bench_out/r06r/$tag.err; python -c "
import json;d=json.loads(open('bench_out/r06r/$tag.json').read().strip().splitlines()[-1]);print('$tag',d['value'],d['ms_per_step'],d['roofline']['us_per_round'],d['parity_gate']['ok'])"; }
for i in 1 2; do
run shipped_d2_$i X=1
run shipped_d3_$i X=1 --geometry-depth 3
run prio1_d2_$i DPM_LIB=$B/libdpm_prio1.so
run prio1_d3_$i DPM_LIB=$B/libdpm_prio1.so --geometry-depth 3
run prio3_d3_$i DPM_LIB=$B/libdpm_prio3.so --geometry-depth 3
done
