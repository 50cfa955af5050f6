"""The CLI's `spam` mode is parsed like the reference's modes: it needs only --in, a missing file fails with `Failed to load X` before the
device is opened, and anything else is a usage error.  No GPU needed."""
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


def test_missing_file_fails_like_the_other_modes(cli, tmp_path):
    missing = str(tmp_path / "missing.png")
    r = run("spam", "--in", missing)
    assert (r.returncode, r.stdout, r.stderr) == (1, "", "Failed to load %s\n" % missing)
    e = run("extract", "--in", missing, "--pass", "p")
    assert (r.returncode, r.stdout, r.stderr) == (e.returncode, e.stdout, e.stderr)


def test_spam_without_in_is_a_usage_error(cli):
    for args in (("spam",), ("spam", "--in"), ("spam", "--out", "x.png")):
        r = run(*args)
        assert r.returncode == 1 and r.stdout == "" and r.stderr.startswith("Usage:"), (args, r.stderr)
    r = run("spam", "--frobnicate", "1")
    assert r.returncode == 1 and r.stderr.startswith("Unknown arg: --frobnicate\nUsage:")


def test_usage_mentions_the_mode(cli):
    r = run("help-me")
    assert r.returncode == 1 and r.stdout == "" and "turtlefft spam" in r.stderr and "--in image.png" in r.stderr


def test_an_unknown_mode_still_prints_usage(cli, tmp_path):
    r = run("spamm", "--in", str(tmp_path / "missing.png"))
    assert r.returncode == 1 and r.stdout == "" and r.stderr.startswith("Usage:")
    for mode in ("gen-key", "embed", "extract"):
        assert "turtlefft %s" % mode in r.stderr
