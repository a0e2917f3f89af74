"""CPU: the pair word as the bucket finish reads it (gfa2network_amd/csrc/g2n_symword.h, shared by
k_sym_finish and this check), compiled for the host under ASan + UBSan as a stand-alone program
(tests/native/symword_check.cpp): a word cut to the 16 bits the last partition pass writes gives the
same two rows as the 32-bit word, for every `low` 1..8 and every pass-1 word layout
(shift1 + low <= 26 bits) after pass 7 has spent its digit.
"""
import os
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_pair_word_cut_to_16_bits_under_asan_ubsan(tmp_path):
    exe = tmp_path / "symword_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", str(ROOT / "tests" / "native" / "symword_check.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([str(exe)], env=env, capture_output=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert r.stdout.startswith(b"symword OK "), r.stdout[-2000:]
