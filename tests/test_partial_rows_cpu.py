"""partial_rows._PartialRows -- the owner of the deferred row sums -- on CPU tensors with a stand-in library: which gradients it takes for
pending slices of a partial-row buffer (exact storage, offset and size), and that settle() raises when a slice handed out by a
backward did not come back from autograd as that very view (a parameter reached twice, a tensor hook)."""
import pytest
import torch

from pmx import partial_rows

FLOATS = 9                              # floats per row: dw [2][3] at 0, db [3] at 6
SLICES = ((0, 6), (6, 3))
ROWS = 2


class StubLib:
    """pmx_defer_row_sums / pmx_last_partial_rows of the library, with a chosen number of partial rows."""

    def __init__(self, rows=ROWS):
        self.rows, self.deferred, self.switched = rows, 0, 0

    def pmx_defer_row_sums(self, on):
        self.deferred, self.switched = on, self.switched + 1
        return 0

    def pmx_last_partial_rows(self):
        return self.rows


@pytest.fixture
def pr():
    """A fresh owner in place of the module's, so that the autograd function below and the test talk to the same one."""
    old, partial_rows.OWNER = partial_rows.OWNER, partial_rows._PartialRows()
    yield partial_rows.OWNER
    partial_rows.OWNER = old


class _Affine(torch.autograd.Function):
    """y = sum(x * w) + sum(b) whose backward returns the parameter gradients as views of row 0 of a partial-row buffer, the way the
    pmx_* backward wrappers do: rows 1 .. ROWS hold the parts, row 0 is NOT summed (NaN) while the sums are deferred."""
    lib = StubLib()

    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x)
        return (x * w).sum() + b.sum()

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        grad = torch.empty((1 + ROWS) * FLOATS)
        wanted = [sl for sl, need in zip(SLICES, ctx.needs_input_grad[1:3]) if need]
        with partial_rows.OWNER.defer(_Affine.lib, grad, FLOATS, wanted, family="stub_affine"):
            full = torch.cat([(dy * x).reshape(-1), dy.expand(3)])
            rows = grad.view(1 + ROWS, FLOATS)
            rows[1], rows[2] = 0.25 * full, 0.75 * full
            rows[0] = float("nan") if _Affine.lib.deferred else full
        return None, grad[0:6].view(2, 3), grad[6:9]


def _params():
    torch.manual_seed(0)
    return torch.randn(2, 3), torch.randn(2, 3, requires_grad=True), torch.randn(3, requires_grad=True)


def _pending_buffer(pr, lib=None, slices=SLICES, **kw):
    """One backward call's worth of bookkeeping without autograd: -> the buffer that is now pending."""
    grad = torch.zeros((1 + ROWS) * FLOATS)
    with pr.defer(lib or StubLib(), grad, FLOATS, slices, **kw):
        pass
    return grad


def test_single_use_claims_every_slice_and_settles(pr):
    x, w, b = _params()
    with pr.enabled(True):
        gw, gb = torch.autograd.grad(_Affine.apply(x, w, b), [w, b])
    assert not pr.on and len(pr.pending) == 1
    assert bool(torch.isnan(gw).all())                                  # row 0 really is unsummed: only the gather may read it
    assert pr.claim(gw.reshape(-1)) == (ROWS, FLOATS) and pr.claim(gb.reshape(-1)) == (ROWS, FLOATS)
    pr.settle()
    assert pr.pending == []


def test_outside_the_enable_context_the_backward_sums_itself_and_nothing_is_pending(pr):
    x, w, b = _params()
    before = _Affine.lib.switched
    gw, gb = torch.autograd.grad(_Affine.apply(x, w, b), [w, b])
    assert pr.pending == [] and _Affine.lib.switched == before           # the library was never told to defer
    assert torch.equal(gw, x) and torch.equal(gb, torch.ones(3))
    assert pr.claim(gw.reshape(-1)) == (0, 0)
    pr.settle()


def test_only_wanted_slices_are_listed(pr):
    x, w, b = _params()
    b = b.detach()                                                       # needs_input_grad[2] is False: db is not listed
    with pr.enabled(True):
        (gw,) = torch.autograd.grad(_Affine.apply(x, w, b), [w])
    assert pr.claim(gw.reshape(-1)) == (ROWS, FLOATS)
    pr.settle()


def test_reshape_of_a_two_dimensional_view_still_claims(pr):
    with pr.enabled(True):
        grad = _pending_buffer(pr)
    dw = grad[0:6].view(2, 3)
    assert pr.claim(dw.reshape(-1)) == (ROWS, FLOATS) and pr.claim(grad[6:9]) == (ROWS, FLOATS)
    pr.settle()


def test_tensors_that_are_not_the_views_do_not_claim_and_settle_raises(pr):
    with pr.enabled(True):
        grad = _pending_buffer(pr, family="stub_family")
    assert pr.claim(grad[0:6].clone()) == (0, 0)                         # equal values, another storage
    assert pr.claim(grad[0:5]) == (0, 0) and pr.claim(grad[6:8]) == (0, 0)   # a listed offset, another size
    assert pr.claim(grad[1:7]) == (0, 0)                                 # inside row 0, but no slice that was handed out
    assert pr.claim(grad[0:6].to(torch.bfloat16)) == (0, 0)
    assert pr.claim(grad[0:12:2]) == (0, 0)                              # a listed offset and size, not contiguous
    assert pr.claim(grad[6:9]) == (ROWS, FLOATS)
    with pytest.raises(RuntimeError, match=r"stub_family.*offset 0 \(6 floats\)"):
        pr.settle()
    assert pr.pending == []                                              # forgotten all the same: the next call starts clean
    pr.settle()


def test_a_parameter_reached_twice_claims_nothing_and_settle_names_the_slice(pr):
    x, w, b = _params()
    with pr.enabled(True):
        gw, gb = torch.autograd.grad(_Affine.apply(x, w, b) + _Affine.apply(2 * x, w, b), [w, b])
    assert len(pr.pending) == 2                                          # two buffers for the same parameters ...
    assert pr.claim(gw.reshape(-1)) == (0, 0) and pr.claim(gb.reshape(-1)) == (0, 0)   # ... and autograd offers their sum
    with pytest.raises(RuntimeError, match=r"stub_affine.*offset 0 \(6 floats\).*reached twice.*hook.*_backward_group"):
        pr.settle()


def test_a_tensor_hook_on_a_parameter_makes_settle_raise(pr):
    x, w, b = _params()
    b.register_hook(lambda g: 2 * g)
    with pr.enabled(True):
        gw, gb = torch.autograd.grad(_Affine.apply(x, w, b), [w, b])
    assert pr.claim(gw.reshape(-1)) == (ROWS, FLOATS)
    assert pr.claim(gb.reshape(-1)) == (0, 0)                            # what the hook returned was computed from an unsummed row 0
    with pytest.raises(RuntimeError, match=r"stub_affine.*offset 6 \(3 floats\)"):
        pr.settle()


def test_an_exception_inside_defer_records_nothing_and_switches_the_library_back(pr):
    lib = StubLib()
    with pr.enabled(True):
        with pytest.raises(ValueError):
            with pr.defer(lib, torch.zeros(27), FLOATS, SLICES):
                assert lib.deferred == 1
                raise ValueError("the kernel call failed")
        assert lib.deferred == 0 and pr.pending == []


def test_casts_or_no_partial_rows_record_nothing(pr):
    lib = StubLib()
    with pr.enabled(True):
        _pending_buffer(pr, lib, plain=False)                            # cast copies leave, not views: the backward sums itself
        assert lib.switched == 0 and pr.pending == []
        _pending_buffer(pr, StubLib(rows=0))                             # the kernel wrote row 0 directly
        assert pr.pending == []


def test_the_enable_context_restores_the_previous_state_and_starts_clean(pr):
    assert pr.on is False
    with pr.enabled(True):
        assert pr.on is True
        _pending_buffer(pr)
        with pr.enabled(False):
            assert pr.on is False and pr.pending == []                   # emptied on entry
            _pending_buffer(pr)
            assert pr.pending == []
        assert pr.on is True
    assert pr.on is False
    with pytest.raises(ZeroDivisionError):
        with pr.enabled(True):
            1 / 0
    assert pr.on is False
