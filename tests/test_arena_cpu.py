"""The arena of tests/helpers.py (guard bands, poisoned gaps, two canaries) checked on its own, without a GPU: plain torch-CPU
stand-ins for a kernel `out[m, :n] = 2 * x[m, :n] + 1` on row-strided views (ld > n), each doing ONE thing wrong.  Every planted
defect must be reported, and the correct stand-in must pass - otherwise tests/test_abi_footprint_gpu.py proves nothing."""
import pytest
import torch

from tests.helpers import ARENA_GUARD, Arena, arena_runs

M, N, LD_X, LD_O = 5, 7, 11, 9


def _x():
    return torch.arange(M * N, dtype=torch.float32).reshape(M, N) / 8 - 2


class _raw:
    """the memory behind a view as the stand-in kernel's pointer sees it: element 0 = the view's first element"""

    def __init__(self, v):
        self.mem = v.region

    def __getitem__(self, i):
        return self.mem[ARENA_GUARD + i]

    def __setitem__(self, i, val):
        self.mem[ARENA_GUARD + i] = val


def correct(x, out, but=None):
    for m in range(M):
        for j in range(N):
            if (m, j) != but:
                out[m * LD_O + j] = 2 * x[m * LD_X + j] + 1


def writes_into_a_gap(x, out):
    correct(x, out)
    out[2 * LD_O + N] = 0.0                        # the float behind row 2


def writes_past_the_end(x, out):
    correct(x, out)
    out[(M - 1) * LD_O + N] = 3.0                  # the float behind the last row: outside the view


def writes_in_front(x, out):
    correct(x, out)
    out[-1] = 3.0


def skips_an_element(x, out):
    correct(x, out, but=(3, 4))                    # a bound one too tight: element (3, 4) is never written


def reads_a_gap(x, out):
    correct(x, out)
    out[LD_O + 2] = 2 * x[LD_X + N] + 1            # a column index one too far: the poison behind row 1 of x


def depends_on_old_contents(x, out):
    old = float(out[4 * LD_O + 1])
    correct(x, out)
    out[4 * LD_O + 1] += 0 if old != old else old * 1e-30       # "+=" into uninitialised memory


def modifies_its_input(x, out):
    correct(x, out)
    x[0] = 9.0


def run(kernel):
    def case(ar):
        x = ar.view("x", (M, N), strides=(LD_X, 1), data=_x())
        out = ar.view("out", (M, N), strides=(LD_O, 1), role="out")
        kernel(_raw(x), _raw(out))
    return arena_runs(case, "cpu", capacity=1 << 20)


def test_correct_stand_in_passes():
    nan, big, differ, _ = run(correct)
    assert not nan.stray and not big.stray and not nan.unwritten and not big.unwritten and not differ
    assert torch.equal(nan.out["out"], 2 * _x() + 1)


@pytest.mark.parametrize("kernel,view,offset", [(writes_into_a_gap, "out", 2 * LD_O + N), (writes_past_the_end, "out", (M - 1) * LD_O + N),
                                                (writes_in_front, "out", -1)])
def test_stray_writes_are_reported(kernel, view, offset):
    nan, big, differ, _ = run(kernel)
    assert nan.stray == {view: (1, offset)} and big.stray == {view: (1, offset)}
    assert not nan.unwritten and not differ


def test_skipped_element_is_reported():
    nan, big, differ, _ = run(skips_an_element)
    assert nan.unwritten == {"out": 1} and big.unwritten == {"out": 1}
    assert differ == ["out"] and not nan.stray
    want = 2 * _x() + 1
    want[3, 4] = float("nan")
    assert torch.equal(nan.out["out"].isnan(), want.isnan()) and torch.equal(nan.out["out"].nan_to_num(), want.nan_to_num())


def test_gap_read_is_reported():
    nan, big, differ, _ = run(reads_a_gap)
    assert differ == ["out"] and torch.isnan(nan.out["out"][1, 2]) and not nan.stray
    assert not big.unwritten                       # (arithmetic keeps a NaN's payload: the NaN run may count the element as unwritten too)


def test_dependence_on_old_contents_is_reported():
    nan, big, differ, _ = run(depends_on_old_contents)
    assert differ == ["out"] and not nan.stray and not nan.unwritten


def test_modified_input_is_reported():
    nan, big, differ, _ = run(modifies_its_input)
    assert "x" in nan.stray and "x" in big.stray


def test_integer_and_double_views_and_partial_promises():
    """int32 / int64 / byte / float64 views carry their own poison; a `promised` mask narrows what must be written, the rest of
    the view then counts as a gap; scratch may be written anywhere inside, not outside."""
    def case(ar, bad):
        idx = ar.view("idx", (6,), torch.int64, role="out", promised=torch.tensor([1, 1, 1, 0, 0, 1], dtype=torch.bool))
        flag = ar.view("flag", (3, 2), torch.uint8, strides=(4, 1), role="out")
        work = ar.view("work", (10,), torch.float64, role="scratch")
        cnt = ar.view("cnt", (2,), torch.int32, data=[5, 6], role="inout")
        idx.t[:3] = 7
        idx.t[5] = -1
        flag.t.fill_(1)
        work.t[3] = 0.5
        cnt.t += 1
        if bad == "unpromised":
            idx.t[3] = 0
        if bad == "scratch":
            work.region[ARENA_GUARD + 10] = 0.0
        if bad == "short":
            flag.t[2, 1] = ar.poison(torch.uint8)
    nan, big, differ, _ = arena_runs(lambda ar: case(ar, None), "cpu", capacity=1 << 20)
    assert not nan.stray and not nan.unwritten and not differ and nan.out["cnt"].tolist() == [6, 7]
    assert arena_runs(lambda ar: case(ar, "unpromised"), "cpu", capacity=1 << 20)[0].stray == {"idx": (1, 3)}
    assert arena_runs(lambda ar: case(ar, "scratch"), "cpu", capacity=1 << 20)[0].stray == {"work": (1, 10)}
    assert arena_runs(lambda ar: case(ar, "short"), "cpu", capacity=1 << 20)[0].unwritten == {"flag": 1}
