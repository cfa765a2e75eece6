"""The poisoned child run that every operator family's GPU test ends with, in one place.

Parent side: ``run_module`` starts ``python -m MODULE --json PATH`` in a fresh process under AMT_DEBUG_POISON=1 and returns
what it wrote; ``assert_unmoved`` compares the child's digests with this process's.  A child that aborted, was killed by
any signal or ran into a time limit ends the whole pytest session (``verdict``): the card may have faulted, and nothing
more is started on it.

Child side: ``poisoned()`` is the one reading of AMT_DEBUG_POISON, ``write`` dumps the result with it, ``digest`` hashes an
array with its dtype and shape.  Not collected by pytest (no test_ prefix), no fixture, no plugin."""
from __future__ import annotations

import hashlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# an abort (SIGABRT), a segmentation fault (SIGSEGV) and a time limit (timeout's 124 and 137), as a shell or as
# subprocess reports them
STOP_STATUSES = (134, -6, 139, -11, 124, 137)


def verdict(returncode: int) -> str:
    """"ok" for 0; "stop" for STOP_STATUSES and for every negative status (death by a signal); "fail" otherwise."""
    if returncode == 0:
        return "ok"
    if returncode in STOP_STATUSES or returncode < 0:
        return "stop"
    return "fail"


def run_module(module: str, json_path, timeout_s: float, what: str, args=()) -> dict:
    """Run ``python -m module --json json_path *args`` from the repository root under AMT_DEBUG_POISON=1 and return its
    JSON.  ``what`` names the run in messages ("the poisoned table").  A time limit or a "stop" status ends the session;
    any other failure raises AssertionError with the child's last output."""
    import pytest  # here, so that a child needs no pytest

    cmd = [sys.executable, "-m", module, "--json", str(json_path), *args]
    env = dict(os.environ, AMT_DEBUG_POISON="1")
    try:
        child = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout_s)
    except subprocess.TimeoutExpired as e:
        pytest.exit(f"{what} did not end within {timeout_s} s; the last output:\n"
                    f"{(e.stdout or b'')[-2000:]!r}\n{(e.stderr or b'')[-2000:]!r}", returncode=1)
    tail = (child.stdout[-3000:] + "\n" + child.stderr[-3000:]).strip()
    v = verdict(child.returncode)
    if v == "stop":
        # an abort, a death by a signal or a time limit: the card may have faulted, nothing more is started on it
        pytest.exit(f"{what} ended with status {child.returncode}; the last output:\n{tail}", returncode=1)
    if v == "fail":
        raise AssertionError(f"{what} ended with status {child.returncode}; the last output:\n{tail}")
    with open(json_path) as f:
        res = json.load(f)
    assert res["poison"] is True
    return res


def assert_unmoved(here: dict, there: dict) -> None:
    """Both runs have the same keys, and every digest of this process equals the poisoned child's."""
    assert set(here) == set(there)
    moved = [k for k in here if here[k] != there[k]]
    assert not moved, f"{len(moved)} results depend on what the scratch held; the first: {moved[:10]}"


def poisoned() -> bool:
    """Whether the library poisons scratch and allocations in this process (it reads the variable's first character)."""
    return os.environ.get("AMT_DEBUG_POISON", "")[:1] == "1"


def write(json_path, res: dict) -> None:
    res["poison"] = poisoned()
    with open(json_path, "w") as f:
        json.dump(res, f)


def digest(a) -> str:
    a = np.ascontiguousarray(a)
    return hashlib.sha256(str(a.dtype).encode() + str(a.shape).encode() + a.tobytes()).hexdigest()
