"""The decode engine's four-value granules of the ffn vector (web-rwkv-gguf_amd/csrc/wrk_ffn_granule.h), on the CPU.

K5 hands relu(k)^2 to K6 as 64-bit granules of four f16 whose sign bits -- provably 0 in the payload -- carry the 4-bit tag
(layer % 15) + 1.  tests/host/eng_ffn_granule_main.cpp includes the HIP-free header alone and goes through all of
it: every one of the 2^15 sign-clear f16 patterns in each of the four positions under every tag.  It is built with the host compiler under
the address and undefined-behaviour sanitizers, linked into the program: a stand-alone executable that runs the same whatever the
environment preloads.  The same properties are static_asserts of the header, so the library's own build fails on a broken tag function.

The layout is restated twice, never through the header's functions: in the program, and here for the dumped granules."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "the host compiler g++ is required"
    exe = str(tmp_path_factory.mktemp("eng_ffn_granule") / "eng_ffn_granule")
    cmd = [cxx, "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "web-rwkv-gguf_amd", "csrc"), "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-Wall", "-Werror", "-g",
           os.path.join(ROOT, "tests", "host", "eng_ffn_granule_main.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([exe], capture_output=True, text=True)
    assert ran.returncode == 0, ran.stdout[-2000:] + ran.stderr
    return json.loads(ran.stdout)


def test_every_sign_clear_f16_round_trips_in_every_position_under_every_tag(report):
    assert report["round_trips"] == 15 * 4 * 2 ** 15
    assert report["bad_pack"] == 0          # the granule is the stated layout
    assert report["bad_payload"] == 0       # unpack returns the payload bit for bit (+0, +inf and the NaN encodings included)
    assert report["no_match"] == 0          # and matches its own tag
    assert report["wrong_match"] == 0       # no other tag, 0 included
    assert report["mask_leak"] == 0         # the producer masks the signs it is handed


def test_a_flipped_sign_bit_never_matches(report):
    assert report["flip_match"] == 0


def test_zero_and_the_previous_layer_never_match(report):
    assert report["layers"] == 64
    assert report["bad_tag"] == 0 and report["zero_match"] == 0
    assert report["prev_checked"] == 63 * 2 ** 15 and report["prev_match"] == 0


def test_granules_equal_the_stated_layout(report):
    """Element e in bits [16 e, 16 e + 16); bit 15 of element e is bit e of (layer % 15) + 1.  33 layers: the tag wraps twice."""
    sample = [0x3C00, 0x7BFF, 0x0001, 0x7C00]
    assert [l for l, _ in report["samples"]] == list(range(33))
    for layer, got in report["samples"]:
        tag = layer % 15 + 1
        want = 0
        for e, h in enumerate(sample):
            want |= (h | (((tag >> e) & 1) << 15)) << (16 * e)
        assert int(got, 16) == want, (layer, got)
