"""A child for tests/test_host_poison_child.py: ``python -m tests.poison_child_stub --json PATH MODE`` behaves as MODE
says.  A plain CPU process: it never imports the package.  Not collected by pytest (no test_ prefix)."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import poison_child  # noqa: E402


def main(argv):
    path, mode = argv[argv.index("--json") + 1], argv[-1]
    print(f"stub out {mode}", flush=True)
    print(f"stub err {mode}", file=sys.stderr, flush=True)
    if mode == "ok":
        poison_child.write(path, {"env": dict(os.environ), "argv": argv[1:]})
    elif mode == "unpoisoned":
        with open(path, "w") as f:
            json.dump({"poison": False}, f)
    elif mode == "exit3":
        return 3
    elif mode == "sleep":
        time.sleep(60)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
