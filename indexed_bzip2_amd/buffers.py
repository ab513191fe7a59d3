"""Many independent bzip2 buffers in one GPU batch: decompress, decompress_many, decompress_many_to_tensor, and the
other way round: compress, compress_many.

Each buffer is a complete .bz2 byte string (a ZIP member stored with method 12, a block of an Avro or Hadoop file, one
blob per sample) and decodes to what ``open(io.BytesIO(buffer), parallelization=1).read()`` returns, stream-CRC check
included.  All buffers of a call share the GPU launches (C: mi355x_bz2_decompress_buffers).

The decoder context of a device is created by the first call for that device and kept for the process (behind a lock,
one call at a time per device): later calls create no context, streams or threads.  ``device=-1`` means torch's current
device once torch has initialised the GPU, else device 0; every function resolves it the same way, so they share the
device's one context.
"""
import sys
import threading

from . import _native as N

_contexts = {}
_lock = threading.Lock()


def _device_index(device: int) -> int:
    """The device ordinal that `device` (-1: the current one) stands for."""
    if device >= 0:
        return device
    torch = sys.modules.get("torch")
    if torch is not None and torch.cuda.is_initialized():
        return torch.cuda.current_device()
    return 0


def _decoder(device: int):
    """(the kept Decoder of `device`, its lock); created on first use."""
    device = _device_index(device)
    with _lock:
        entry = _contexts.get(device)
        if entry is None:
            entry = (N.Decoder(device=device), threading.Lock())
            _contexts[device] = entry
        return entry


def _run(buffers, device, max_launch_blocks):
    if max_launch_blocks < 0:
        raise ValueError("max_launch_blocks must not be negative")
    dec, lock = _decoder(device)
    lock.acquire()
    try:
        results, total = dec.decompress_buffers(buffers, max_launch_blocks)
    except BaseException:
        lock.release()
        raise
    return dec, lock, results, total


def _statuses(results):
    import numpy as np
    return np.array([r["status"] for r in results], dtype=np.int32)


def _raise_first_failure(results):
    for i, r in enumerate(results):
        if r["status"] != N.OK:
            raise N.Bz2Error(r["status"], f"buffer {i}, status {r['status']}, at bit offset {r['error_offset_bits']}")


def decompress_many(buffers, device: int = -1, max_launch_blocks: int = 0, return_status: bool = False):
    """Decode every buffer (bytes, bytearray, memoryview, numpy uint8: any C-contiguous buffer) -> list of bytes.

    Blocks of all buffers are decoded together, in launches of at most `max_launch_blocks` (0 = 512).  A failed buffer
    raises Bz2Error naming its index, status and bit offset; with ``return_status=True`` nothing raises and the result
    is ``(list of bytes, numpy int32 statuses)`` with failed buffers empty.  Uses the device's kept decoder context
    (created by the first call for the device, never by later ones)."""
    buffers = list(buffers)
    if not buffers:
        import numpy as np
        return ([], np.zeros(0, dtype=np.int32)) if return_status else []
    dec, lock, results, total = _run(buffers, device, max_launch_blocks)
    try:
        if not return_status:
            _raise_first_failure(results)
        blob = dec.copy_output(0, total) if total else b""
    finally:
        lock.release()
    out = [blob[r["output_offset"]:r["output_offset"] + r["decoded_size"]] for r in results]
    return (out, _statuses(results)) if return_status else out


def decompress(data, device: int = -1) -> bytes:
    """One buffer: what bz2.decompress(data) returns, with the reader's rules where they differ (listed at
    mi355x_bz2_decompress_buffers in include/mi355x_bz2.h: trailing garbage is ignored, "BZh9" alone is empty).
    Uses the device's kept decoder context."""
    return decompress_many([data], device=device)[0]


def decompress_many_to_tensor(buffers, device: int = -1, max_launch_blocks: int = 0, return_status: bool = False):
    """Decode every buffer into ONE contiguous torch.uint8 tensor on the GPU -> (data, offsets): buffer i is
    ``data[offsets[i]:offsets[i + 1]]``; `offsets` is an int64 CPU tensor of n + 1 boundaries.  The decoded bytes never
    pass through the host.  Failures as in decompress_many (with ``return_status=True``: ``(data, offsets, statuses)``,
    failed buffers empty).  Uses the device's kept decoder context."""
    import torch
    buffers = list(buffers)
    torch.cuda.init()
    dev = _device_index(device)
    if not buffers:
        data = torch.empty(0, dtype=torch.uint8, device=f"cuda:{dev}")
        offsets = torch.zeros(1, dtype=torch.int64)
        if return_status:
            import numpy as np
            return data, offsets, np.zeros(0, dtype=np.int32)
        return data, offsets
    dec, lock, results, total = _run(buffers, dev, max_launch_blocks)
    try:
        if not return_status:
            _raise_first_failure(results)
        data = torch.empty(total, dtype=torch.uint8, device=f"cuda:{dev}")
        if total:
            # the new tensor's memory may still be in use by work queued on torch's stream: the copy comes after it
            torch.cuda.current_stream(data.device).synchronize()
            dec.gather_output_to_device([(0, 0, total)], data.data_ptr())
    finally:
        lock.release()
    bounds = [0]
    for r in results:
        bounds.append(bounds[-1] + r["decoded_size"])
    offsets = torch.tensor(bounds, dtype=torch.int64)
    return (data, offsets, _statuses(results)) if return_status else (data, offsets)


def compress_many(buffers, compresslevel: int = 9, device: int = -1, max_launch_blocks: int = 0,
                  return_index: bool = False):
    """Compress every buffer (bytes, bytearray, memoryview, numpy uint8: any C-contiguous buffer; empty ones too) into
    one complete single-stream .bz2 each -> list of bytes.  ``bz2.decompress`` and ``decompress_many`` give the buffer
    back.  `compresslevel` 1..9 means what it means to bzip2 (blocks of 100k x level), and the blocks are cut exactly
    where libbz2 cuts them; the encoded bits may differ from libbz2's.  Blocks of all buffers are encoded together on
    the GPU, in launches of at most `max_launch_blocks` (0 = 512); the output does not depend on it.
    With ``return_index=True`` the result is a list of ``(bytes, offsets)``: `offsets` is the block map
    ``open(io.BytesIO(out), 0).block_offsets()`` would build, ready for ``set_block_offsets`` / ``write_block_offsets``.
    Uses the device's kept context (created by the first call for the device, never by later ones)."""
    if isinstance(compresslevel, bool) or not isinstance(compresslevel, int) or not 1 <= compresslevel <= 9:
        raise ValueError("compresslevel must be an integer from 1 to 9")
    if max_launch_blocks < 0:
        raise ValueError("max_launch_blocks must not be negative")
    buffers = list(buffers)
    if not buffers:
        return []
    dec, lock = _decoder(device)
    with lock:
        results, total = dec.compress_buffers(buffers, compresslevel, max_launch_blocks)
        blob = dec.copy_output(0, total) if total else b""
        maps = [dec.compress_block_map(i) for i in range(len(buffers))] if return_index else None
    out = [blob[r["output_offset"]:r["output_offset"] + r["compressed_size"]] for r in results]
    return list(zip(out, maps)) if return_index else out


def compress(data, compresslevel: int = 9, device: int = -1) -> bytes:
    """One buffer: a .bz2 stream that bz2.decompress turns back into `data` (see compress_many).  Uses the device's
    kept context."""
    return compress_many([data], compresslevel=compresslevel, device=device)[0]
