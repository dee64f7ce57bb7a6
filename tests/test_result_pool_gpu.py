"""The library's result-buffer pool (hy_result_pool_*, csrc/result_pool.hip), which holds every device-resident PosList behind
_on_execute(): blocks handed out again, releases it refuses, where a pair's two lists lie, trim, calibration (the pairs it keeps, and
nothing left behind when the join refuses), and a release from a thread of another device.  The pool is process-wide and other tests
leave blocks in it, so every test trims first and asserts on differences of hy_result_pool_stats."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from hyrise_amd import abi
from hyrise_amd.storage import DeviceColumn
from support import build_column

pytestmark = pytest.mark.gpu
MiB = 1 << 20


def stats(lib):
    held, in_use, calibrated = C.c_uint64(), C.c_uint64(), C.c_uint32()
    abi.check(lib.hy_result_pool_stats(C.byref(held), C.byref(in_use), C.byref(calibrated)))
    return held.value, in_use.value, calibrated.value


def acquire(lib, nbytes):
    ptr = C.c_void_p()
    abi.check(lib.hy_result_pool_acquire(nbytes, C.byref(ptr)))
    return ptr.value


def acquire_pair(lib, rows):
    left, right = C.c_void_p(), C.c_void_p()
    abi.check(lib.hy_result_pool_acquire_pair(rows, C.byref(left), C.byref(right)))
    return left.value, right.value


def release(lib, *pointers):
    for ptr in pointers:
        abi.check(lib.hy_result_pool_release(ptr))


@pytest.fixture
def pool(device):
    abi.check(device.hy_result_pool_trim())
    yield device
    abi.check(device.hy_result_pool_trim())


def small_join(n=20_000):
    """A key column with n unique keys and a probe column of 3n keys that each match once: 3n pairs."""
    rng = np.random.default_rng(7)
    build = build_column(rng.permutation(np.arange(n, dtype=np.int32)), None, 4096, abi.ENC_UNENCODED)
    probe = build_column(rng.integers(0, n, 3 * n).astype(np.int32), None, 8192, abi.ENC_UNENCODED)
    return DeviceColumn(build), DeviceColumn(probe), 3 * n


def test_a_released_block_is_handed_out_again(pool):
    wanted = 3 * MiB
    held0, used0, _ = stats(pool)
    ptr = acquire(pool, wanted)
    held1, used1, _ = stats(pool)
    usable = held1 - held0
    assert ptr % (2 * MiB) == 0 and wanted + 2 * MiB < usable <= wanted + 4 * MiB
    assert used1 - used0 == usable
    release(pool, ptr)
    assert stats(pool)[:2] == (held1, used0)
    assert acquire(pool, wanted) == ptr
    assert stats(pool)[:2] == (held1, used1)
    release(pool, ptr)
    assert stats(pool)[:2] == (held1, used0)


def test_release_refuses_what_the_caller_does_not_hold(pool):
    ptr = acquire(pool, 4096)
    release(pool, ptr)
    assert pool.hy_result_pool_release(ptr) == abi.ERR_INVALID              # a second time
    assert pool.hy_result_pool_release(ptr + 256) == abi.ERR_INVALID        # never handed out
    assert pool.hy_result_pool_release(None) == abi.OK


def test_the_lists_of_a_pair_start_apart_on_the_2mib_grid(pool):
    rows = 100_000
    held0, used0, _ = stats(pool)
    left, right = acquire_pair(pool, rows)
    assert left % (2 * MiB) == 0
    assert right % (2 * MiB) == 5 * MiB // 4
    held1, used1, _ = stats(pool)
    assert used1 - used0 == held1 - held0 >= 2 * 8 * rows
    release(pool, left, right)
    assert stats(pool)[:2] == (held1, used0)
    assert acquire_pair(pool, rows) == (left, right)   # taken again, both lists together
    assert stats(pool)[:2] == (held1, used1)
    release(pool, left, right)


def test_trim_frees_every_idle_block(pool):
    held_kept = stats(pool)[0]
    kept = acquire(pool, MiB)
    idle = [acquire(pool, 4096), acquire(pool, 5 * MiB), *acquire_pair(pool, 50_000)]
    release(pool, *idle)
    abi.check(pool.hy_result_pool_trim())
    held, used, _ = stats(pool)
    assert held == used and held - held_kept >= MiB
    release(pool, kept)
    abi.check(pool.hy_result_pool_trim())
    assert stats(pool)[0] == held_kept


@pytest.mark.parametrize("flags, kept", [(0, 1), (abi.POOL_KEEP_MEDIAN, 2)])
def test_calibrate_keeps_the_fastest_pair(pool, flags, kept):
    left, right, rows = small_join()
    held0, used0, calibrated0 = stats(pool)
    times = (C.c_float * 2)()
    chosen = C.c_uint32(99)
    abi.check(pool.hy_result_pool_calibrate(left.handle, right.handle, abi.JOIN_INNER, rows, 2, flags, times, C.byref(chosen)))
    held, used, calibrated = stats(pool)
    assert chosen.value in (0, 1) and all(t > 0 for t in times)
    assert calibrated - calibrated0 == kept
    assert used == used0   # the kept pairs are free
    assert kept * 2 * 8 * rows < held - held0 <= kept * (2 * 8 * rows + 8 * MiB)
    pair = acquire_pair(pool, rows)   # a kept pair, not a new one
    assert stats(pool)[0] == held and stats(pool)[1] > used
    release(pool, *pair)


def test_calibrate_over_a_refused_join_leaves_the_pool_as_it_was(pool):
    # JoinHash refuses a full outer join before any launch: every candidate pair is already allocated by then
    left, right, rows = small_join()
    before = stats(pool)
    assert pool.hy_result_pool_calibrate(left.handle, right.handle, abi.JOIN_FULL_OUTER, rows, 4, 0, None, None) == abi.ERR_UNSUPPORTED
    assert stats(pool) == before


def test_release_from_a_thread_of_another_device(pool):
    count = C.c_int32(0)
    abi.check(pool.hy_device_count(C.byref(count)))
    if count.value < 2:
        pytest.skip("one visible device")
    workers = {d: ThreadPoolExecutor(1) for d in (0, 1)}

    def on(d, f, *args):
        return workers[d].submit(f, *args).result()

    try:
        for d in workers:
            abi.check(on(d, pool.hy_bind_device, d))
        abi.check(on(1, pool.hy_result_pool_trim))
        held0, used0, _ = stats(pool)
        ptr = on(1, acquire, pool, 2 * MiB)
        held1, used1, _ = stats(pool)
        assert used1 - used0 == held1 - held0 > 0
        abi.check(on(0, pool.hy_result_pool_release, ptr))
        assert stats(pool)[:2] == (held1, used0)
        assert on(1, acquire, pool, 2 * MiB) == ptr
        abi.check(on(1, pool.hy_result_pool_release, ptr))
        abi.check(on(1, pool.hy_result_pool_trim))
        assert stats(pool)[:2] == (held0, used0)
    finally:
        for worker in workers.values():
            worker.submit(pool.hy_shutdown).result()
            worker.shutdown()
