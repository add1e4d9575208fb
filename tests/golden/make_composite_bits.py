"""Records tests/golden/composite_bits.json: a SHA-256 per output tensor of every case of
tests/test_gpu_composite_bits.py (the compositors, their NULL-argument forms and nslam_render_loss on the
seeded cases of tests/ray_edge_cases.py).

Run on a GPU with the library of the commit whose bits are the reference.  Build that commit in a separate
checkout and point NSLAM_LIB at its libnslam.so:

    NSLAM_LIB=/path/to/parent/nice-slam_amd/libnslam.so \
        python tests/golden/make_composite_bits.py PARENT_COMMIT "$(hipcc --version | grep 'HIP version')" [OUT.json]

The commit hash and the compiler line are stored as plain information.  Each case is run twice and must repeat
itself before it is written.  The committed file was recorded at the parent of the commit that folded the
occupancy, density and loss compositing into one templated compositor.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, os.path.dirname(TESTS))
sys.path.insert(0, TESTS)

import test_gpu_composite_bits as cb  # noqa: E402


def main():
    commit, hipcc = sys.argv[1], sys.argv[2]
    out = sys.argv[3] if len(sys.argv) > 3 else cb.BITS
    digests = {}
    for name in cb.CASES:
        digests[name] = {k: cb.digest(v) for k, v in cb.run_case(name)[0].items()}
        again = {k: cb.digest(v) for k, v in cb.run_case(name)[0].items()}
        if again != digests[name]:
            raise SystemExit(f"{name}: the run does not repeat")
        print(name, " ".join(sorted(digests[name])))
    with open(out, "w") as f:
        json.dump({"parent_commit": commit, "hipcc": hipcc, "digests": digests}, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
