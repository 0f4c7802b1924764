"""Records what the C ABI's entry points answer to the bad arguments of tests/abi_refusal_cases.py: return code and qr_last_error()
of every case, written to tests/golden/abi_refusals.json.  Needs an MI355X.

    python tools/record_abi_refusals.py [--out PATH]

The file pins the ORDER of the refusals across a change of the host code, so it is recorded from the library as it was BEFORE that
change (build the parent commit's csrc/, run this, then change the code); it is not regenerated afterwards.  A new entry point adds
its cases to the table and is recorded the same way, from the commit that introduced it."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    import abi_refusal_cases as A

    out = os.path.join(ROOT, "tests", "golden", "abi_refusals.json")
    if "--out" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1]
    results, touched = A.run_cases()
    if touched:
        sys.exit("a refused call wrote something: %s" % touched)
    accepted = [name for name, (rc, _) in results.items() if rc == 0]
    if accepted:
        sys.exit("not refused: %s" % accepted)
    with open(out, "w") as f:
        json.dump(results, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d cases -> %s" % (len(results), out))


if __name__ == "__main__":
    main()
