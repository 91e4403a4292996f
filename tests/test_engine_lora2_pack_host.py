"""The decode engine's packed LoRA-2 image (web-rwkv-gguf_amd/csrc/wrk_lora2_pack.h), on the CPU.

tests/host/eng_lora2_pack_main.cpp includes the HIP-free header alone, packs four synthetic matrices with the engine's own packer and reads
the image back the way a head workgroup does: piece (head, u, n) at the offset the kernel computes, lane L's 16 bytes into register n.  It
is built with the host compiler under the address and undefined-behaviour sanitizers, linked into the program: a stand-alone executable
that runs the same whatever the environment preloads.

What a lane's register must hold is restated twice, never through the header's own source functions: in the program from the kernel's
loads before the pack (row head * 64 + 16 bi + (L >> 2), columns 8 (L & 3) + 32 n .. + 8 of matrix u / 4), and here, for the dumped
images, from the layout as DESIGN.md section 4.8 states it.  Piece counts, bytes and unit offsets are worked out here from the ranks."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (w, a, v, g) as the model's description lists them; the image's matrix order is w, a, g, v
RANKS = [(96, 96, 64, 256), (40, 24, 8, 72), (128, 128, 128, 256), (8, 8, 8, 8)]
HEADS = [4, 32]


def elem(m, row, col):
    return (((m * 7919 + row * 131 + col * 17) << 1) | 1) & 0xFFFF


@pytest.fixture(scope="module")
def packer(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "the host compiler g++ is required"
    exe = str(tmp_path_factory.mktemp("eng_lora2_pack") / "eng_lora2_pack")
    cmd = [cxx, "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "web-rwkv-gguf_amd", "csrc"), "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-Wall", "-Werror", "-g",
           os.path.join(ROOT, "tests", "host", "eng_lora2_pack_main.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr

    def run(cases):
        """cases: [(name, H, (w, a, v, g), has_v, row_pad, dump)] -> one record per case"""
        lines = [f"{name} {H} {w} {a} {g} {v} {int(has_v)} {pad} {int(dump)}" for name, H, (w, a, v, g), has_v, pad, dump in cases]
        ran = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert ran.returncode == 0, ran.stdout[-2000:] + ran.stderr
        out = [json.loads(line) for line in ran.stdout.splitlines()]
        assert len(out) == len(cases), ran.stderr
        return out
    return run


def pieces(rank):
    return -(-rank // 32)


@pytest.mark.parametrize("H", HEADS)
@pytest.mark.parametrize("ranks", RANKS)
def test_every_element_once_where_the_kernel_reads_it(packer, ranks, H):
    w, a, v, g = ranks
    order = (w, a, g, v)
    for has_v, pad in ((True, 0), (False, 16)):
        p = packer([("c", H, ranks, has_v, pad, False)])[0]
        pph = 4 * sum(pieces(r) for r in order)
        assert p["pieces_per_head"] == pph
        # offsets 1 KB-aligned and dense: every piece of the image is the piece of exactly one (head, u, n), none lies outside
        assert p["bytes"] == H * pph * 1024
        assert p["misaligned"] == 0 and p["out_of_image"] == 0 and p["twice"] == 0 and p["pieces_unused"] == 0
        # units of a head in the order of u, each a run of its matrix's pieces
        want, at = [], 0
        for u in range(16):
            want.append(at)
            at += pieces(order[u // 4])
        assert p["unit_piece"] == want + [pph]
        # every element (row, col < rank) exactly once, at the lane and register of the kernel's mapping (zeros for layer 0's v2)
        assert p["elements"] == H * 64 * sum(order)
        assert p["not_once"] == 0 and p["mismatches"] == 0
        # no piece with 32 n >= rank; the lanes beyond the rank are zero
        assert p["beyond_rank"] == 0
        assert p["pad_lanes"] == H * 4 * 16 * sum(4 * pieces(r) - r // 8 for r in order)
        assert p["pad_nonzero"] == 0


def test_1p5b_is_64_kb_per_head_and_2_mb_per_layer(packer):
    p = packer([("1p5b", 32, (96, 96, 64, 256), True, 0, False)])[0]
    assert p["pieces_per_head"] == 64 and p["bytes"] == 2 << 20
    assert p["unit_piece"][:5] == [0, 3, 6, 9, 12] and p["unit_piece"][8] == 24 and p["unit_piece"][12] == 56


@pytest.mark.parametrize("has_v", [True, False])
def test_image_equals_the_stated_layout(packer, has_v):
    """Partial last pieces (40, 72), a matrix below 32 columns (24), the minimum rank (8); rows 16 bytes further apart than their rank."""
    ranks = (40, 24, 8, 72)
    w, a, v, g = ranks
    order = (w, a, g, v)
    H = 4
    p = packer([("dump", H, ranks, has_v, 16, True)])[0]
    got = np.frombuffer(bytes.fromhex(p["image"]), dtype="<u2")
    want = []
    for head in range(H):
        for u in range(16):
            mi, bi = divmod(u, 4)
            n = 0
            while 32 * n < order[mi]:                               # pieces with 32 n >= rank do not exist
                for lane in range(64):
                    row, c = head * 64 + 16 * bi + (lane >> 2), 8 * (lane & 3) + 32 * n
                    for e in range(8):
                        want.append(elem(mi, row, c + e) if c < order[mi] and (mi < 3 or has_v) else 0)
                n += 1
    want = np.array(want, dtype="<u2")
    assert got.shape == want.shape
    assert np.array_equal(got, want)
