#!/bin/bash
# What the driver runs at the end of a round: the GPU suite, smoke(), the --full bench line (summary printed).
python -m pytest tests -m gpu -x -q > gpurun_out/r3_t14.log 2>&1; tail -2 gpurun_out/r3_t14.log
python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -1
LINE=$(python bench.py --full 2>/dev/null | grep '^{' | tail -1) python - <<'PY'
import json, os
d = json.loads(os.environ["LINE"])
print(d["value"], d["ms_per_step"], d["roofline"]["frac"], d["roofline"]["stale"], d["cpu_baseline"]["value"],
      {k: (v.get("value") if isinstance(v, dict) else None) for k, v in d["secondary"].items()})
PY
