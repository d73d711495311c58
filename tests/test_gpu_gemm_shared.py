"""The split-bf16 GEMM's tile rule by stream (option ``g3_shared``, csrc/gemm_choice.hpp): a launch on the device's default stream
is priced by its makespan on an empty chip, a launch on any other stream by its chip time, and ``g3_shared`` = 1 / 2 forces either
rule on any stream.  Every tile variant gives the same bits, so whichever rule a launch gets, the output is the same.

Shapes: the smallest at which the two rules differ on 256 CUs (tests/native/gemm_choice_shared_check.cpp holds the table).
  * 129 tiles of 256 x 256 (M = 11 008, N = 768, K = 768, residual in place): 160-row tiles by makespan, the 8-phase kernel by chip
    time.  Both are one launch, and no hook names the kernel a launch took, so this case asserts bit equality only.
  * the strip case (M = 12 800, N = 3072, K = 768, GELU -> split output): cut at column 2560 by makespan (two launches), uncut by
    chip time (one).  The ``SL_PROF_GEMM`` slot counts the launches, which tells the two rules apart.
"""
import pytest
import torch

from semanticlens_amd import _native as N

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def operands():
    g = torch.Generator(device=DEV).manual_seed(0)
    K = 768

    def rnd(*s):
        return torch.randn(*s, device=DEV, generator=g)

    ops = {
        "x129": N.Split.of(rnd(11008, K)), "w768": N.Split.of(rnd(768, K) * 0.03), "b768": rnd(768), "res": rnd(11008, 768),
        "x": N.Split.of(rnd(12800, K)), "w3072": N.Split.of(rnd(3072, K) * 0.03), "b3072": rnd(3072),
    }
    torch.cuda.synchronize()
    return ops


def _residual_case(o):
    out = o["res"].clone()
    N.linear3(o["x129"], o["w768"], o["b768"], residual=out, out=out)
    return [out]


def _strip_case(o):
    sp = N.Split(12800, 3072, DEV)
    N.linear3(o["x"], o["w3072"], o["b3072"], act=N.SL_ACT_GELU, out_split=sp)
    return [sp.hi.view(torch.int16), sp.lo.view(torch.int16)]


def _run(case, o, shared, side):
    """Outputs (on the host) and the number of GEMM launches of one call under option g3_shared = `shared`, on a side stream or
    on the default stream."""
    assert torch.cuda.current_stream().cuda_stream == 0  # the tests run on the default stream: the library sees handle 0
    N.set_option("g3_shared", shared)
    N.prof_enable(True)
    N.prof_reset()
    try:
        if side:
            st = torch.cuda.Stream()
            st.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(st):
                assert torch.cuda.current_stream().cuda_stream != 0
                outs = case(o)
            torch.cuda.current_stream().wait_stream(st)
        else:
            outs = case(o)
        _, launches, _ = N.prof_read(N.SL_PROF_GEMM)
        torch.cuda.synchronize()
        return [t.cpu() for t in outs], launches
    finally:
        N.prof_enable(False)
        N.prof_reset()
        N.set_option("g3_shared", 0)


# (g3_shared, side stream) -> the rule the launch gets
WAYS = [(0, False, "makespan"), (0, True, "chip"), (1, False, "makespan"), (1, True, "makespan"), (2, False, "chip"), (2, True, "chip")]


def test_residual_gemm_of_129_tiles_is_the_same_on_every_stream_and_rule(operands):
    want, launches = _run(_residual_case, operands, 1, False)
    assert launches == 1
    for shared, side, _ in WAYS:
        got, n = _run(_residual_case, operands, shared, side)
        assert n == 1, (shared, side)
        assert torch.equal(got[0], want[0]), (shared, side)


def test_strip_gemm_is_cut_by_makespan_and_whole_by_chip_time(operands):
    want, launches = _run(_strip_case, operands, 1, False)
    assert launches == 2  # columns [0, 2560) and the 512-column strip
    for shared, side, rule in WAYS:
        got, n = _run(_strip_case, operands, shared, side)
        assert n == (2 if rule == "makespan" else 1), (shared, side, n)
        for a, b in zip(got, want):
            assert torch.equal(a, b), (shared, side)
