"""hc_mont_lazy (csrc/hc_arith.h): the product of a lazy 64-bit x with a fixed operand held as ONE 8-byte Montgomery word, which hc_k_b5m's epilogue uses for idx and the key's Q rows
instead of 16-byte Shoup pairs. The header is compiled for the host as it stands (a three-line shim, g++) and checked against Python's big integers on the worst cases; then the
kernel that uses it runs in the fibre emulator against the oracle on a tree that small_levels = 0 sends through b1 .. b4 and hc_k_b5m at every level."""
import ctypes
import os
import random
import subprocess

import pytest

import parity_cases as pc
from oracle_lib import P0, Q0, Q1

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "optimal_conv_amd", "csrc")
M64 = (1 << 64) - 1
EMU_DIR = os.path.join(ROOT, "tests", "kernel_emu")
EMU_LIB = os.path.join(EMU_DIR, "_build", "libhconv_emu.so")

SHIM = """
#include "hc_arith.h"
extern "C" uint64_t t_mont_lazy(uint64_t x, uint64_t wm, uint64_t q, uint64_t qinv) { return hc_mont_lazy(x, wm, q, qinv); }
extern "C" uint64_t t_mont(uint64_t a, uint64_t b, uint64_t q, uint64_t qinv) { return hc_mont(a, b, q, qinv); }
"""

# Q0 (2^55: the FREE branch of hc_k_b5m, Q0 < 2^57), the 60-bit and 61-bit primes the chain tests use (the ALT branch: no lazy headroom), and the 49-bit Q1
MODULI = [Q0, pc.Q1_BL, P0, Q1]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("mont_shim")
    src, so = os.path.join(d, "shim.cpp"), os.path.join(d, "libshim.so")
    open(src, "w").write(SHIM)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", CSRC, "-o", so, src])
    L = ctypes.CDLL(so)
    for f in (L.t_mont_lazy, L.t_mont):
        f.restype = ctypes.c_uint64
        f.argtypes = [ctypes.c_uint64] * 4
    return L


@pytest.mark.parametrize("q", MODULI, ids=lambda q: f"q{q.bit_length()}")
def test_mont_lazy_against_big_integers(shim, q):
    assert 2 * q < 1 << 64
    qinv = pow(q, -1, 1 << 64)
    rng = random.Random(q)
    # x: every 64-bit value is allowed - the extremes, the lazy bounds of the epilogue (2q, 4q: hc_shoup4 / hc_fold results; 6q, 81q: the FREE-mode sums), their neighbours
    xs = [0, 1, q - 1, q, q + 1, M64, M64 - 1, 1 << 63, (1 << 63) - 1, (1 << 32) - 1, 1 << 32]
    for k in (2, 4, 6, 8, 72, 81, 83):
        xs += [v for v in (k * q - 1, k * q, k * q + 1) if v <= M64]
    xs += [rng.getrandbits(64) for _ in range(200)]
    ws = [q - 1, q - 2, 1, 0, 2, (q - 1) // 2, (q + 1) // 2] + [rng.randrange(q) for _ in range(40)]
    for w in ws:
        wm = (w << 64) % q
        assert shim.t_mont(w, pow(2, 128, q), q, qinv) == wm            # how the tables are built on the device: hc_k_pointwise<HC_PW_TO_MONT>
        for x in xs:
            r = shim.t_mont_lazy(x, wm, q, qinv)
            assert r % q == x * w % q, (hex(x), hex(w))
            assert 0 < r < 2 * q, (hex(x), hex(w), hex(r))                # the stated bound: [1, 2q - 1], inside hc_shoup4's [0, 4q)


def test_free_mode_headroom_of_the_b5m_epilogue():
    """the FREE branch (Q0 < 2^57) with both products below 2q: t1 = y + m + bias < 4q ; T = fold(y + 4q - m) < 4q needs y + 4q - m < 8q ; f = y + 4q - m + g + 72q - n with
    n < 70q is positive and below 79q ; the one hc_reduce64 takes t1 + f < 83q, which must fit 64 bits"""
    q = (1 << 57) - 1                                                     # the largest modulus the FREE branch accepts is below this
    y, m_lo, m_hi, g_hi, n_hi = q - 1, 1, 2 * q - 1, 2 * q - 1, 70 * q - 1
    assert y + 4 * q - m_lo < 8 * q and 0 - m_hi + 4 * q > 0
    assert 0 + 4 * q - m_hi + 1 + 72 * q - n_hi > 0                      # smallest f
    f_hi = y + 4 * q - m_lo + g_hi + 72 * q
    assert f_hi < 79 * q
    assert (y + m_hi + (q - 1)) + f_hi < 83 * q < 1 << 64


@pytest.mark.parametrize("max_ob,chunk", [(8, None), (4, 2)])
def test_conv_then_pack_through_b5m_in_the_emulator(max_ob, chunk):
    """hc_k_b5m with the 8-byte operand tables (hc_idx_load / hc_evk_load build them) == the oracle, bit for bit: small_levels = 0 keeps every tree level on b1 .. b4, b5m"""
    from optimal_conv_amd import Context
    from oracle_lib import Oracle
    subprocess.check_call(["make", "-s", "-C", EMU_DIR, EMU_LIB])
    ctx = Context([Q0, Q1], [P0], lib_path=EMU_LIB)
    try:
        ctx.set_option("small_levels", 0)
        pc.case_conv(ctx, Oracle(), max_ob, chunk=chunk)
    finally:
        ctx.close()
