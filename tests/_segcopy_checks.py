"""The checks of mrz_copy_device_batch (mrz_seg_copy_kernel, modern-rzip_amd/csrc/mrz_segcopy.hip), shared by the
emulator tier (test_segcopy_emu.py) and the GPU tier (test_segcopy_gpu.py).  Every destination lies in one buffer that is
pre-filled with a guard byte and compared whole with what numpy copies, so a byte written outside a segment fails."""
import ctypes

import numpy as np
import pytest
import torch

import modern_rzip_amd as m

E_ARG = -1
TILE = 16384   # MRZ_SEG_TILE
GUARD = 0xA5
SYMBOLS = ("mrz_copy_device_batch",)


def check_abi(lib):
    assert lib.mrz_abi_version() == 4
    assert all(hasattr(lib, s) for s in SYMBOLS)


def _buffers(src_bytes, dst_len, emu):
    """-> (source tensor, destination tensor, their 16-byte aligned base offsets): device memory, guard-filled target"""
    dev = "cpu" if emu else "cuda"
    src = torch.zeros(len(src_bytes) + 32, dtype=torch.uint8, device=dev)
    dst = torch.full((dst_len + 32,), GUARD, dtype=torch.uint8, device=dev)
    sb, db = (-src.data_ptr()) % 16, (-dst.data_ptr()) % 16
    src[sb:sb + len(src_bytes)] = torch.frombuffer(bytearray(src_bytes), dtype=torch.uint8).to(dev)
    return src, dst, sb, db


def run(ctx, emu, src_bytes, dst_len, segs):
    """segs: (offset in the source, offset in the destination, length), offsets counted from 16-byte aligned bases.
    Copies them in one call and compares the whole destination buffer."""
    src, dst, sb, db = _buffers(src_bytes, dst_len, emu)
    want = np.full(dst_len + 32, GUARD, dtype=np.uint8)
    data = np.frombuffer(src_bytes, dtype=np.uint8)
    for so, do, n in segs:
        assert 0 <= so and so + n <= len(src_bytes) and 0 <= do and do + n <= dst_len
        want[db + do:db + do + n] = data[so:so + n]
    ctx.copy_device_batch([(src.data_ptr() + sb + so, dst.data_ptr() + db + do, n) for so, do, n in segs])
    got = dst.cpu().numpy()
    if not np.array_equal(got, want):
        k = int(np.nonzero(got != want)[0][0]) - db
        raise AssertionError(f"destination byte {k}: got {got[k + db]}, want {want[k + db]} ({len(segs)} segments)")


def noise(n, seed):
    return np.random.default_rng(seed).integers(0, 256, size=n, dtype=np.uint8).tobytes()


LENGTHS = (0, 1, 15, 16, 17, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 5)


def check_lengths(ctx, emu, src_mis, dst_mis):
    """every listed length, each alone and all of them in one call, destinations end to end from a destination that is
    dst_mis bytes off a 16-byte boundary, sources src_mis bytes off"""
    data = noise(3 * TILE + 64, 1)
    for n in LENGTHS:
        run(ctx, emu, data, n + 48, [(src_mis, dst_mis, n)])
    segs, at = [], dst_mis
    for k, n in enumerate(LENGTHS):
        segs.append((src_mis + (k % 3), at, n))
        at += n
    run(ctx, emu, data, at + 16, segs)


def check_misalignments(ctx, emu):
    """all 256 pairs of source and destination misalignment at length 100, in one call: the 16-byte, the 4-byte and the
    byte path, each with every head and tail length"""
    data = noise(4096, 2)
    segs, at = [], 0
    for sa in range(16):
        for da in range(16):
            at = (at + 15) // 16 * 16 + da + 16   # a guard gap in front of every destination
            segs.append((16 * sa + sa, at, 100))
            at += 100
    run(ctx, emu, data, at + 16, segs)


def check_shared_source(ctx, emu):
    """two destinations from one source, and two sources that overlap"""
    data = noise(3000, 3)
    run(ctx, emu, data, 8000, [(7, 0, 2500), (7, 2500, 2500), (1000, 5000, 2000), (5, 7001, 0), (0, 7100, 900)])


def check_many_segments(ctx, emu):
    """300 segments of random lengths 0..200 in one call: several workgroups, searches that diverge between them"""
    rng = np.random.default_rng(4)
    data = noise(1 << 16, 5)
    segs, at = [], 3
    for _ in range(300):
        n = int(rng.integers(0, 201))
        segs.append((int(rng.integers(0, len(data) - n + 1)), at, n))
        at += n
    assert sum(1 for s in segs if s[2] == 0) >= 1
    run(ctx, emu, data, at + 16, segs)


def check_arguments(ctx, emu):
    lib = ctx.lib
    src, dst, sb, db = _buffers(b"x" * 64, 64, emu)
    vp, i64 = ctypes.c_void_p, ctypes.c_int64

    def rc(srcs, dsts, lens, n=None):
        k = len(lens)
        return lib.mrz_copy_device_batch(ctx.ctx, (vp * max(k, 1))(*srcs), (vp * max(k, 1))(*dsts),
                                         (i64 * max(k, 1))(*lens), k if n is None else n)

    s, d = src.data_ptr(), dst.data_ptr()
    assert rc([], [], []) == 0 and lib.mrz_copy_device_batch(ctx.ctx, None, None, None, 0) == 0
    assert lib.mrz_copy_device_batch(ctx.ctx, None, None, None, 1) == E_ARG
    assert lib.mrz_copy_device_batch(None, None, None, None, 0) == E_ARG
    assert rc([s], [d], [8], n=-1) == E_ARG
    assert rc([s, s], [d, d + 8], [8, -1]) == E_ARG      # a negative length: nothing is copied
    assert rc([s, None], [d, d + 8], [8, 1]) == E_ARG    # a null pointer with a positive length
    assert rc([s, s], [d, None], [8, 1]) == E_ARG
    assert bytes(dst.cpu().numpy()) == bytes([GUARD]) * (64 + 32)
    assert rc([None, s], [None, d], [0, 8]) == 0         # ... with a length of zero it is not looked at
    with pytest.raises(m.MrzError) as e:
        ctx.copy_device_batch([(s, d, -5)])
    assert e.value.rc == E_ARG
