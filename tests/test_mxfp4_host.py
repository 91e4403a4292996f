"""GGUF tensor type 39 (ggml block_mxfp4: u8 e; u8 qs[16] per 32 elements) in the host reader: size accounting and the f16 dequantiser."""
import struct

import numpy as np
import pytest

import wrk

E2M1 = np.array([0, .5, 1, 1.5, 2, 3, 4, 6, -0., -.5, -1, -1.5, -2, -3, -4, -6])


def _gguf(dims, data: bytes) -> bytes:
    """Minimal GGUF v3 with one type-39 tensor whose data is `data`."""
    def wstr(s):
        return struct.pack("<Q", len(s)) + s.encode()

    head = bytearray(struct.pack("<IIQQ", 0x46554747, 3, 1, 1))
    head += wstr("general.architecture") + struct.pack("<I", 8) + wstr("rwkv7")
    head += wstr("blk.0.time_mix_key.weight") + struct.pack("<I", len(dims)) + b"".join(struct.pack("<Q", d) for d in dims) + struct.pack("<IQ", 39, 0)
    return bytes(head) + b"\0" * (-len(head) % 32) + data


def test_type_39_reads_back_as_the_dequantised_blocks():
    k, m = 96, 4
    r = np.random.default_rng(39)
    blocks = r.integers(0, 256, (k // 32 * m, 17), dtype=np.uint8)
    blocks[:8, 0] = [0, 1, 102, 110, 127, 140, 143, 255]          # below, inside and above what f16 holds
    blocks[0, 1:9] = [0x10, 0x32, 0x54, 0x76, 0x98, 0xBA, 0xDC, 0xFE]
    codes = np.concatenate([blocks[:, 1:] & 15, blocks[:, 1:] >> 4], axis=1)
    with np.errstate(over="ignore"):
        want = (E2M1[codes] * np.exp2(blocks[:, :1].astype(np.float64) - 127)).astype(np.float16).reshape(-1)
    reader = wrk.GgufReader(_gguf([k, m], blocks.tobytes()))
    got = reader.tensor_f16("blocks.0.att.key.weight").view(np.float16)
    assert np.array_equal(got.view(np.uint16), want.view(np.uint16))


def test_truncated_type_39_tensor_is_refused():
    with pytest.raises(wrk.WrkError):
        wrk.GgufReader(_gguf([96, 4], b"\0" * (12 * 17 - 1)))
