"""What hso_gpu_debug_wave_primitives (include/hso_gpu_debug.h) must return, from the contracts stated in hso_amd/csrc/hso_wave.h,
in numpy.  Shared by tests/test_wave_gpu.py (the device library) and tests/test_abi_cpu.py (tests/fakegpu's restatement).  The
inputs are small integers that depend on thread and index, so every sum is exact in fp32 and fp64 and the comparison is equality."""
import numpy as np

THREADS, VALUES, FIELDS = 128, 32, 32
# field offsets (enum of include/hso_gpu_debug.h)
BUTTERFLY_F64, BUTTERFLY_F32, BUTTERFLY_I32, TO_LANE63_F64, TO_LANE63_I32 = 0, 1, 2, 3, 4
XOR_F64, XOR_F32, SCAN_I32, HALVE32_F64, HALVE32_F32, HALVE8_F64 = 5, 11, 17, 18, 20, 22
ROW16_F32, ROW8_F32, SWAP32_F64, SWAP16_F32, SHFL_F64, SHFL_XOR_F64, SHFL_XOR_I64 = 24, 25, 26, 27, 28, 29, 30


def inputs():
    t, i = np.mgrid[0:THREADS, 0:VALUES]
    return ((t * 37 + i * 11) % 97 - 48).astype(np.float64)


def check(values, out):
    """values, out: float64 [128, 32].  Asserts every field of every lane, wavefront by wavefront."""
    assert out.shape == (THREADS, FIELDS) and values.shape == (THREADS, VALUES)
    lane = np.arange(64)
    for wave in range(THREADS // 64):
        v, o = values[64 * wave:64 * wave + 64], out[64 * wave:64 * wave + 64]   # [lane, index], [lane, field]
        tot = v.sum(axis=0)                                                       # wave total of every index
        assert np.array_equal(o[:, BUTTERFLY_F64], np.full(64, tot[0]))
        assert np.array_equal(o[:, BUTTERFLY_F32], np.full(64, tot[1]))
        assert np.array_equal(o[:, BUTTERFLY_I32], np.full(64, tot[2]))
        assert o[63, TO_LANE63_F64] == tot[3] and o[63, TO_LANE63_I32] == tot[4]
        for k in range(6):
            assert np.array_equal(o[:, XOR_F64 + k], v[lane ^ (32 >> k), 5]), 32 >> k
            assert np.array_equal(o[:, XOR_F32 + k], v[lane ^ (32 >> k), 6]), 32 >> k
        assert np.array_equal(o[:, SCAN_I32], np.cumsum(v[:, 7]))
        # the halving contract: slot = lane / G for G = 64 / N adjacent lanes, every lane of a slot holds the slot's total,
        # every slot < N is held
        for field, n in ((HALVE32_F64, 32), (HALVE32_F32, 32), (HALVE8_F64, 8)):
            g = 64 // n
            assert np.array_equal(o[:, field], lane // g), (field, "slot")
            assert sorted(set(o[:, field])) == list(range(n))
            assert np.array_equal(o[:, field + 1], tot[lane // g]), (field, "total")
        assert np.array_equal(o[:, ROW16_F32], v[:, 8].reshape(4, 16).sum(axis=1).repeat(16))
        assert np.array_equal(o[:, ROW8_F32], v[:, 9].reshape(8, 8).sum(axis=1).repeat(8))
        for field, m in ((SWAP32_F64, 32), (SWAP16_F32, 16)):
            idx = np.where(lane & m, 11, 10)                                      # lower lanes: lo + lo', upper lanes: hi + hi'
            assert np.array_equal(o[:, field], v[lane, idx] + v[lane ^ m, idx]), m
        assert np.array_equal(o[:, SHFL_F64], v[(5 * lane + 3) % 64, 12])
        assert np.array_equal(o[:, SHFL_XOR_F64], v[lane ^ (21 << wave), 12])
        assert np.array_equal(o[:, SHFL_XOR_I64], v[lane ^ (21 << wave), 12])
