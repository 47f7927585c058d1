"""GPU: a few rounds of the seeded differential fuzz of the kernels around the encoder against their numpy models
(tests/stage_fuzz.py), one test per stage at the committed seed.  IIV_STAGE_FUZZ_SIDE_STREAM=1 runs the same rounds with all
device work on a non-blocking side stream (as IIV_FUZZ_SIDE_STREAM does for tests/fuzz_parity.py)."""
import os

import pytest

import stage_fuzz

pytestmark = pytest.mark.gpu
SIDE_STREAM = os.environ.get("IIV_STAGE_FUZZ_SIDE_STREAM") == "1"
ROUNDS = 12


def _rounds(stage):
    """ROUNDS for every stage but the chain, which runs 4"""
    return stage_fuzz.ROUNDS[stage]


@pytest.mark.parametrize("stage", stage_fuzz.STAGES)
def test_stage_equals_its_model(native, stage):
    done = stage_fuzz.run(_rounds(stage), stage_fuzz.SEED, [stage], side_stream=SIDE_STREAM)
    assert len(done) == _rounds(stage)
