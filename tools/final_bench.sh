O=${1:-out/final_bench}
mkdir -p $O
timeout 1500 python bench.py --full > $O/bench.json 2> $O/bench.err
timeout 600 python bench.py --full --mode exact_f32 --no-encoders --no-other-path > $O/bench_exact.json 2>> $O/bench.err
python - <<PY
import json
d=json.loads(open("$O/bench.json").read().strip().split("\n")[-1])
print(d["value"], d["ms_per_step"], d["roofline"]["frac"], d["roofline"]["kernel_ms"])
s=d["secondary"]
print("dpr", s["dpr"]["ms_per_batch"], "clip", s["clip"]["ms_per_batch"], "small", s["small_batch"]["ms"], s["small_batch"]["scan_kernel_ms"])
print("l2", json.dumps(s.get("small_batch_l2"))[:700])
print("map_arrow", json.dumps(s["reference_call_surface"].get("map_arrow"))[:300])
PY
