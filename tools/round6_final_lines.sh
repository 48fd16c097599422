# bash tools/round6_final_lines.sh OUTDIR  on the GPU machine, AFTER tools/round6_digest.sh was run and its profiles/r06_* committed: the bench lines of the final
# tree with counters / mix / parity record filled (--full; the digests are keyed by the source hash) + the rocprofv3 --kernel-trace --stats summary of the driver's default command
O=$(realpath -m "${1:?usage: round6_final_lines.sh OUTDIR}")
R=$(realpath "$(dirname "$0")/..")
cd "$R"
mkdir -p "$O"
python bench.py --full > "$O/bench.json" 2> "$O/bench.err"
python bench.py --workload c2 > "$O/bench_c2.json" 2> "$O/bench_c2.err"
python bench.py --workload c5 > "$O/bench_c5.json" 2> "$O/bench_c5.err"
python bench.py --full --per-pixel-ht --no-e2e > "$O/bench_c3b.json" 2> "$O/bench_c3b.err"
(cd /tmp && TMPDIR=/tmp timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d "$O/kt" -- python "$R/bench.py" > "$O/bench_under_rocprof.json" 2> "$O/kt.err")
python - "$O/bench.json" <<'PY'
import json, sys
d=json.load(open(sys.argv[1])); r=d['roofline']
print('value', d['value']/1e9, 'ms', d['ms_per_step'], 'march', r['march_ms_per_step'], 'cross', r['crossings_ms_per_step'], 'frac', r['frac'], 'busy', r['valu_busy_frac'], 'clock', r['clock_GHz_measured'])
print({k: r[k] for k in ('executed_fp64_flops_frac','useful_flops_frac','survey_flops_frac_step','survey_bytes_over_hbm_peak_step','frac_class_priced','frac_at_measured_clock','valu_per_evaluated_sample','frac_hbm_measured','traffic_over_compulsory')})
print(d['parity'])
print({k:(v.get('value'),v.get('ms_per_step')) for k,v in d['secondary'].items() if k in ('c2','c5')}, {k:(v['rays_per_s'], v['valu_per_evaluated_sample']) for k,v in d['secondary']['real_levels'].items()})
PY
