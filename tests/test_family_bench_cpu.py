"""tests/helpers/family_bench.py, the owner of what the stand-alone benchmark scripts share.  The child-per-step driver is what
keeps those scripts safe on a shared card -- after a step that fails or runs out of its time nothing more may be started -- so
it is driven here with a stub script whose steps print, fail, oversleep or leave a marker; and every tests/bench_*.py is checked
to have given its copies up.  No device, no torch."""
import ast
import glob
import json
import os
import subprocess
import sys
import textwrap

import pytest

TESTS = os.path.dirname(os.path.abspath(__file__))
HELPERS = os.path.join(TESTS, "helpers")
sys.path.insert(0, HELPERS)
import family_bench as FB  # noqa: E402

STUB = textwrap.dedent('''\
    import json, os, sys, time
    sys.path.insert(0, %r)
    import family_bench as FB

    def step(name):
        if name == "good":
            print("a line that is not the result")
            print(json.dumps({"step": name, "value": 0.1, "pid": os.getpid()}))
        elif name == "fail":
            print(json.dumps({"step": name}))
            sys.exit(3)
        elif name == "sleep":
            time.sleep(60)
        elif name == "marker":
            open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "marker"), "w").close()
            print(json.dumps({"step": name}))

    if __name__ == "__main__":
        FB.main(__file__, ("good", "marker"), step, lambda results: print("summary", sorted(results)))
    ''') % HELPERS


@pytest.fixture
def stub(tmp_path):
    path = tmp_path / "bench_stub.py"
    path.write_text(STUB)
    return str(path)


def started(stub):
    return os.path.exists(os.path.join(os.path.dirname(stub), "marker"))


def test_a_good_step_prints_and_parses_its_last_line_only(stub, capfd):
    results = FB.run_steps(stub, ("good", "marker"))
    out = capfd.readouterr().out.splitlines()
    assert list(results) == ["good", "marker"] and started(stub)
    assert results["good"]["step"] == "good" and results["good"]["value"] == 0.1 and results["good"]["pid"] != os.getpid()
    assert [json.loads(line) for line in out] == [results["good"], results["marker"]]


def test_a_failing_step_ends_the_run_and_nothing_more_is_started(stub, capfd):
    with pytest.raises(SystemExit) as e:
        FB.run_steps(stub, ("good", "fail", "marker"))
    assert e.value.code == "bench_stub: step fail ended with status 3; nothing more is started"
    assert [json.loads(line)["step"] for line in capfd.readouterr().out.splitlines()] == ["good"]
    assert not started(stub)


def test_a_step_over_its_limit_ends_the_run_and_nothing_more_is_started(stub, capfd):
    with pytest.raises(SystemExit) as e:
        FB.run_steps(stub, ("sleep", "marker"), seconds=1)
    assert e.value.code == "bench_stub: step sleep ran out of its 1 s; nothing more is started"
    assert capfd.readouterr().out == "" and not started(stub)


def test_main_runs_one_named_step_in_this_process(stub, monkeypatch, capfd):
    ran = []
    monkeypatch.setattr(subprocess, "run", lambda *a, **k: pytest.fail("--step must not start a child"))
    monkeypatch.setattr(sys, "argv", [stub, "--step", "fused"])
    FB.main(stub, ("a", "b"), lambda name: ran.append((name, os.getpid())), lambda results: pytest.fail("no summary after --step"))
    assert ran == [("fused", os.getpid())]


def test_a_script_s_command_line(stub):
    """The stub's own ``main`` is one call of family_bench.main: whole, it prints each step's line and then its summary; with
    ``--step`` it prints what the step prints."""
    whole = subprocess.run([sys.executable, stub], stdout=subprocess.PIPE, text=True, timeout=60)
    lines = whole.stdout.splitlines()
    assert whole.returncode == 0 and len(lines) == 3 and lines[2] == "summary ['good', 'marker']"
    assert [json.loads(line)["step"] for line in lines[:2]] == ["good", "marker"]
    one = subprocess.run([sys.executable, stub, "--step", "good"], stdout=subprocess.PIPE, text=True, timeout=60)
    assert one.returncode == 0 and one.stdout.splitlines()[0] == "a line that is not the result"


def test_importing_the_module_imports_no_torch():
    """Not torch, so neither torch.cuda nor a device: the timers and recipes import it when they are called."""
    code = "import sys; sys.path.insert(0, %r); import family_bench; print(sorted(m for m in sys.modules if m.split('.')[0] == 'torch'))"
    done = subprocess.run([sys.executable, "-c", code % HELPERS], stdout=subprocess.PIPE, text=True, timeout=60)
    assert done.returncode == 0 and done.stdout.strip() == "[]"


def test_every_bench_script_compiles_and_has_given_its_copies_up():
    scripts = sorted(glob.glob(os.path.join(TESTS, "bench_*.py")))
    assert len(scripts) >= 22
    for path in scripts:
        text = open(path).read()
        tree = ast.parse(text, path)
        compile(tree, path, "exec")
        for word in ("subprocess.run", "TimeoutExpired"):
            assert word not in text, (path, word)
        defined = {n.name for n in ast.walk(tree) if isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef))}
        assert not defined & {"best_seconds", "timed", "timed_us"}, (path, defined)
        assert "import family_bench" in text or "from family_bench import" in text, path
