#!/usr/bin/env python3
"""What the plugin layer's routes RETURN, for comparing two versions of the Python package over one libturbogp.so: one
line per case of tests/plugin_route_cases.py with a SHA-256 of the chosen point(s), of every key and value of the info
('sweep_ms', a device time, left out) and of ``np.random``'s state afterwards.

    PYTHONPATH=<tree of the other version> TGP_LIBRARY=turbo_amd/csrc/libturbogp.so python tools/plugin_routes_digest.py > a.txt
    TGP_LIBRARY=turbo_amd/csrc/libturbogp.so python tools/plugin_routes_digest.py > b.txt && diff a.txt b.txt

(the repository's own tree comes LAST on the module path here, so that ``PYTHONPATH`` chooses the package.)
``--record-calls FILE`` also writes the ordered ``tgp_*`` entry names of every case as JSON: the golden file of
tests/test_gpu_plugin_routes.py."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(ROOT)
sys.path.append(os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--record-calls", default=None)
    args = ap.parse_args()
    import turbo_amd as ta
    import plugin_route_cases as prc
    print("# package %s" % os.path.relpath(os.path.dirname(os.path.abspath(ta.__file__)), ROOT), file=sys.stderr)
    calls, failed = {}, 0
    for case_id in prc.case_ids():
        try:
            out = prc.run_case(ta, case_id)
        except Exception as e:      # (say which case and go on: the other lines are still worth comparing)
            failed += 1
            print("%-34s FAILED %s: %s" % (case_id, type(e).__name__, e), flush=True)
            continue
        calls[case_id] = out["entries"]
        print(prc.digest_line(case_id, out), flush=True)
    if args.record_calls:
        with open(args.record_calls, "w") as f:
            f.write("{\n" + ",\n".join('  "%s": %s' % (k, json.dumps(v)) for k, v in calls.items()) + "\n}\n")
    print("digest done" if not failed else "digest done, %d cases failed" % failed)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
