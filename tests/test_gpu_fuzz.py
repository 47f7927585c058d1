"""GPU: a few rounds of the randomised differential run (tests/fuzz_parity.py)."""
import os
import runpy

import pytest

pytestmark = pytest.mark.gpu


def test_fuzz_rounds(monkeypatch, capsys):
    monkeypatch.setenv("IIV_FUZZ_ROUNDS", "10")
    monkeypatch.setenv("IIV_FUZZ_SEED", "77")
    runpy.run_path(os.path.join(os.path.dirname(__file__), "fuzz_parity.py"), run_name="__main__")
    assert "all equal" in capsys.readouterr().out


def test_fuzz_rounds_on_a_side_stream(monkeypatch, capsys):
    """the same draws of options with every round's device work on a non-blocking stream (IIV_FUZZ_SIDE_STREAM)"""
    monkeypatch.setenv("IIV_FUZZ_ROUNDS", "6")
    monkeypatch.setenv("IIV_FUZZ_SEED", "1913")
    monkeypatch.setenv("IIV_FUZZ_SIDE_STREAM", "1")
    runpy.run_path(os.path.join(os.path.dirname(__file__), "fuzz_parity.py"), run_name="__main__")
    assert "on a side stream" in capsys.readouterr().out
