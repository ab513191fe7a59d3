"""The stream layout of a batch (csrc/bz2_lanes.hpp) follows the number of contexts alive on the device: the same batch is
decoded while 1, 2, 3, 4 and 5 contexts are alive, so that it runs with block groups on lanes of their own, on shared
lanes, and as one group on the context's stream alone (with the runtime's default of 4 hardware queues: 4, 2, 1, 1 and 1
lanes; with more queues, other splits).  The input of each context's next batch is queued with set_input_host_async while
its batch is in flight, into the context's second input buffer.  Records and decoded bytes must be the same in every
case, and every block's CRC must match."""
import ctypes

import pytest

import datagen

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def workload(native):
    # 300 text blocks and 24 incompressible ones (level 1: 100 kB blocks): enough blocks for cost chunks and an expensive
    # minority when the layout allows groups, few enough for the side-by-side k_mtf instances
    raw_text, raw_random = datagen.text_like(30_000_000, 201), datagen.random_bytes(2_400_000, 202)
    enc = datagen.multistream([raw_text, raw_random], 1)
    offsets = native.find_magic(enc)
    assert len(offsets) >= 300
    return enc, raw_text + raw_random, offsets


def records(arr, n):
    return [arr[k].as_dict() for k in range(n)]


def test_same_batch_with_one_to_five_contexts_alive(native, workload):
    enc, raw, offsets = workload
    n = len(offsets)
    pinned = (ctypes.c_ubyte * len(enc)).from_buffer_copy(enc)     # stays alive and in place
    want = None
    for alive in (1, 2, 3, 4, 5):
        decs = [native.Decoder(max_batch_blocks=n) for _ in range(alive)]
        try:
            arrays = [d.make_arrays(offsets) for d in decs]
            for d in decs:
                d.set_input_host_async(ctypes.addressof(pinned), len(enc), keepalive=pinned)
            # two rounds on every context, batches of all contexts in flight together; the first round queues each
            # context's next input while its batch runs
            for rnd in range(2):
                for d, (offs, _) in zip(decs, arrays):
                    d.begin_batch(offs, n)
                    if rnd == 0:
                        d.set_input_host_async(ctypes.addressof(pinned), len(enc), keepalive=pinned)
                for k, (d, (_, res)) in enumerate(zip(decs, arrays)):
                    total = d.end_batch(res)
                    got = records(res, n)
                    assert total == len(raw), (alive, rnd, k)
                    assert all(r["status"] == 0 and r["computed_crc"] == r["header_crc"] for r in got), (alive, rnd, k)
                    if want is None:
                        want = got
                    assert got == want, (alive, rnd, k)
                    assert d.copy_output(0, total) == raw, (alive, rnd, k)
        finally:
            for d in decs:
                d.close()
