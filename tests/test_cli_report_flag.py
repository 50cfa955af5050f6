"""The CLI's --report flag is parsed like the reference's booleans: accepted (no `Unknown arg`), and a trailing flag without a value is
treated exactly as one of --adaptive_alpha.  Parsing happens before the device is opened: no GPU needed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "steganosaurus_amd", "turtlefft")


def run(*args, cwd=None):
    return subprocess.run([CLI, *args], capture_output=True, text=True, cwd=cwd)


@pytest.fixture(scope="module")
def cli():
    if not os.path.exists(CLI):
        subprocess.run(["make", "-C", os.path.join(ROOT, "steganosaurus_amd", "csrc"), "-j4"], check=True, stdout=subprocess.DEVNULL)
    return CLI


@pytest.mark.parametrize("value", ["1", "true", "0"])
def test_report_is_accepted(cli, tmp_path, value):
    missing = str(tmp_path / "missing.png")
    r = run("embed", "--in", missing, "--out", str(tmp_path / "o.png"), "--secret", "s", "--pass", "p", "--report", value)
    assert "Unknown arg" not in r.stderr
    assert (r.returncode, r.stderr) == (1, "Failed to load %s\n" % missing)


def test_report_without_a_value_is_treated_like_adaptive_alpha(cli, tmp_path):
    missing = str(tmp_path / "missing.png")
    base = ["embed", "--in", missing, "--out", str(tmp_path / "o.png"), "--secret", "s", "--pass", "p"]
    a = run(*base, "--report")
    b = run(*base, "--adaptive_alpha")
    assert (a.returncode, a.stdout, a.stderr) == (b.returncode, b.stdout, b.stderr)
    a = run("embed", "--report", "--in", missing)
    b = run("embed", "--adaptive_alpha", "--in", missing)
    assert (a.returncode, a.stdout, a.stderr) == (b.returncode, b.stdout, b.stderr)


def test_usage_mentions_the_flag(cli):
    r = run("help-me")
    assert r.returncode == 1 and "--report" in r.stderr
