"""The wave64 lane-exchange primitives (hso_amd/csrc/hso_wave.h) by themselves, MI355X: one 128-thread workgroup (two wavefronts,
so a helper that takes the thread index for the lane fails) evaluates every primitive on small integers; tests/wave_ref.py states
what each lane must hold — exact equality, no tolerance — including the halving sum's slot contract as the header words it."""
import pytest

import wave_ref

pytestmark = pytest.mark.gpu


def test_wave_primitives_on_device(gpu_ctx):
    values = wave_ref.inputs()
    wave_ref.check(values, gpu_ctx.debug_wave_primitives(values))
