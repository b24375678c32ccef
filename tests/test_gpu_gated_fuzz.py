"""A short seeded slice of the randomised sentinel parity run of the gated matchers (tests/fuzz_gated.py: hak_match_guided,
hak_match_epipolar and their batch forms against the numpy statements, bit for bit), one test per matcher, plus the cases the
long run (`python tests/fuzz_gated.py --cases 3000 --seed 3`, profiles/fuzz_gated.txt) has failed on, pinned by (seed, index).
What the inputs can catch is asserted without a device in tests/test_gated_fuzz_cpu.py.

HAK_FUZZ_GATED_CASES / HAK_FUZZ_SEED widen the slice (the convention of test_gpu_fuzz.py).  The default walks the first 480
indices of the committed seed, about 240 cases and 13 batch groups per matcher; measured on an MI355X box: 4.2 s (guided) and
3.9 s (epipolar) per test, the numpy statement and the generator being most of it."""
import io
import os

import pytest

import fuzz_gated as fg

pytestmark = pytest.mark.gpu

CASES = int(os.environ.get("HAK_FUZZ_GATED_CASES", "480"))
SEED = int(os.environ.get("HAK_FUZZ_SEED", "3"))
FOUND = []                           # (seed, index) of every case the long run failed on before its fix: none so far


def _slice(matcher):
    out = io.StringIO()
    failed = fg.run(CASES, SEED, verbose=False, out=out, matcher=matcher)
    assert not failed, out.getvalue()
    assert f"{matcher})" in out.getvalue() and ", 0 failed" in out.getvalue()


def test_guided_fuzz_slice(ah):
    _slice("guided")


def test_epipolar_fuzz_slice(ah):
    _slice("epipolar")


@pytest.mark.parametrize("seed,index", FOUND)
def test_cases_the_long_run_found(ah, seed, index):
    out = io.StringIO()
    assert not fg.run(0, seed, only=index, verbose=False, out=out), out.getvalue()
