"""tests/poison_child.py on the host: which statuses of a child end the session, what ``run_module`` hands to its child
and makes of each way the child can end, ``assert_unmoved`` and ``digest``.  The children are tests/poison_child_stub.py,
plain CPU processes; no test sends a signal to anything."""
import os
import subprocess

import numpy as np
import pytest

import poison_child

STUB = "tests.poison_child_stub"


def test_verdict():
    assert poison_child.verdict(0) == "ok"
    assert poison_child.STOP_STATUSES == (134, -6, 139, -11, 124, 137)
    for status in poison_child.STOP_STATUSES + (-7, -9, -4):  # SIGBUS, SIGKILL, SIGILL: every death by a signal
        assert poison_child.verdict(status) == "stop", status
    for status in (1, 2, 3):
        assert poison_child.verdict(status) == "fail", status


@pytest.mark.parametrize("before", [None, "0", "1"])
def test_round_trip(tmp_path, monkeypatch, before):
    monkeypatch.setenv("AMT_STUB_MARKER", "a value of the parent's")
    if before is None:
        monkeypatch.delenv("AMT_DEBUG_POISON", raising=False)
    else:
        monkeypatch.setenv("AMT_DEBUG_POISON", before)
    res = poison_child.run_module(STUB, tmp_path / "out.json", 30, "the stub", args=("ok",))
    assert res["poison"] is True
    assert res["argv"] == ["--json", str(tmp_path / "out.json"), "ok"]
    env = res["env"]
    assert env["AMT_DEBUG_POISON"] == "1" and env["AMT_STUB_MARKER"] == "a value of the parent's"
    assert all(env.get(k) == v for k, v in os.environ.items() if k != "AMT_DEBUG_POISON")
    # nothing else added (LC_CTYPE: the interpreter sets it for itself where the locale is C)
    assert set(env) - set(os.environ) <= {"AMT_DEBUG_POISON", "LC_CTYPE"}
    assert os.environ.get("AMT_DEBUG_POISON") == before  # the parent's own environment stays


def test_a_failing_child_is_an_assertion_error_with_its_output(tmp_path):
    with pytest.raises(AssertionError) as e:
        poison_child.run_module(STUB, tmp_path / "out.json", 30, "the stub", args=("exit3",))
    msg = str(e.value)
    assert "the stub" in msg and "status 3" in msg and "stub out exit3" in msg and "stub err exit3" in msg


def test_an_unpoisoned_child_fails(tmp_path):
    with pytest.raises(AssertionError):
        poison_child.run_module(STUB, tmp_path / "out.json", 30, "the stub", args=("unpoisoned",))


def test_a_time_limit_ends_the_session(tmp_path):
    with pytest.raises(pytest.exit.Exception) as e:
        poison_child.run_module(STUB, tmp_path / "out.json", 1, "the stub", args=("sleep",))
    assert e.value.returncode == 1
    assert "the stub did not end within 1 s" in e.value.msg


@pytest.mark.parametrize("status", [-11, 134, -7])
def test_a_stop_status_ends_the_session(tmp_path, monkeypatch, status):
    seen = {}

    def run(cmd, **kwargs):
        seen.update(kwargs, cmd=cmd)
        return subprocess.CompletedProcess(cmd, status, stdout="x" * 4000 + "last words", stderr="on stderr")

    monkeypatch.setattr(poison_child.subprocess, "run", run)
    with pytest.raises(pytest.exit.Exception) as e:
        poison_child.run_module(STUB, tmp_path / "out.json", 30, "the stub")
    assert e.value.returncode == 1
    msg = e.value.msg
    assert f"the stub ended with status {status}" in msg and "last words" in msg and "on stderr" in msg
    assert msg.count("x") == 3000 - len("last words")  # the last 3000 characters of a stream
    assert seen["cwd"] == poison_child.ROOT and seen["timeout"] == 30 and seen["capture_output"] and seen["text"]
    assert seen["cmd"][1:] == ["-m", STUB, "--json", str(tmp_path / "out.json")]


def test_assert_unmoved():
    here = {"a": "1", ("b", 2): "2"}
    poison_child.assert_unmoved(here, dict(here))
    with pytest.raises(AssertionError, match="1 results depend on what the scratch held; the first: .'a'."):
        poison_child.assert_unmoved(here, dict(here, a="other"))
    with pytest.raises(AssertionError):
        poison_child.assert_unmoved(here, {"a": "1"})  # a key is missing there
    with pytest.raises(AssertionError):
        poison_child.assert_unmoved(here, dict(here, c="3"))  # an extra key there


def test_digest_covers_dtype_and_shape():
    a = np.arange(12, dtype=np.uint8)
    assert poison_child.digest(a) == poison_child.digest(a.copy()) == poison_child.digest(a.reshape(3, 4).T.T.ravel())
    assert poison_child.digest(a) != poison_child.digest(a.view(np.int8))  # equal bytes, another dtype
    assert poison_child.digest(a) != poison_child.digest(a.reshape(3, 4))  # equal bytes, another shape
    assert poison_child.digest(a.reshape(3, 4)) != poison_child.digest(a.reshape(4, 3))
    assert poison_child.digest(a.reshape(3, 4).T) == poison_child.digest(np.ascontiguousarray(a.reshape(3, 4).T))
