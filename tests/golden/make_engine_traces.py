"""Records tests/golden/engine_traces.json: the enqueue trace of every case of tests/test_gpu_engine_trace.py.

Run on a GPU, with nice-slam_amd/engine.py at the commit whose launch order is the reference:

    python tests/golden/make_engine_traces.py [OUT.json]

The committed file was recorded at the parent of the commit that split query_bwd and iteration into a plan,
launchers and a prefetch ring (the cases use only surface that exists on both sides).  Each case is run twice
and must repeat itself before it is written.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, os.path.dirname(TESTS))
sys.path.insert(0, TESTS)

import conftest  # noqa: E402
import test_gpu_engine_trace as tr  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else tr.TRACES
    tiny = conftest.load_golden("tiny_scene")
    traces = {}
    for name in sorted(tr.CASES):
        traces[name] = tr.CASES[name](tiny)
        again = tr.CASES[name](tiny)
        if again != traces[name]:
            raise SystemExit(f"{name}: the trace does not repeat")
        print(name, len(traces[name]), "entries,", len({lab for _, lab in traces[name]}), "streams")
    with open(out, "w") as f:
        rows = [json.dumps(k) + ": " + json.dumps(v, separators=(",", ":")) for k, v in traces.items()]
        f.write("{\n" + ",\n".join(rows) + "\n}\n")  # one case per line


if __name__ == "__main__":
    main()
