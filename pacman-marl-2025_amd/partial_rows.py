"""The deferred row sums of the partial-row gradient buffers: one owner from the backward kernels to the learner's gather.

`OWNER` is the only binding of the single instance.  The kernel wrappers (critic_kernels, actor_head) and PPOLearner reach it as
`partial_rows.OWNER` at call time, so a test that rebinds it swaps the owner for all of them at once."""
import contextlib

import torch

from . import _lib


class _PartialRows:
    """Owner of the deferred row sums.  The backward calls of the pmx_ffn / tok96 / tok32ln / *_tail families end with a small
    second-stage kernel that adds the partial rows of the parameter gradients into row 0 -- a launch on the critic's chain of the
    launch-bound 512-sample step between every two backward kernels, although nothing before the gradient gather reads its result.
    While `enabled` (PPOLearner._backward_group around autograd) the library skips that kernel, the buffer is remembered here with
    the (offset, numel) slices of row 0 it hands out, and the gather (pmx_flatten_sum_to_f32) adds the rows while it copies.  A
    gradient is matched to its buffer EXACTLY -- storage, offset and size -- and `settle` raises unless every slice handed out came
    back: a sum of two unsummed row-0 views, or whatever a hook returned, is wrong before the learner sees it."""

    def __init__(self):
        self.on = False          # True only inside `enabled`; any other caller of the autograd functions gets the summed row 0
        self.pending = []        # [buffer, partial rows, floats per row, family, {(offset, numel): claimed}]

    @contextlib.contextmanager
    def enabled(self, on=True):
        """Deferral on (or off) for the autograd call inside; nothing of an earlier, failed call stays pending."""
        prev, self.on = self.on, bool(on)
        self.pending = []
        try:
            yield self
        finally:
            self.on = prev

    @contextlib.contextmanager
    def defer(self, lib, grad, floats, slices, plain=True, family="partial rows"):
        """Context for ONE backward call.  slices: (offset, numel) of every parameter gradient handed out as a view of row 0 of grad
        and wanted (ctx.needs_input_grad); plain: those views leave as they are, float32 (no cast copies)."""
        on = self.on and plain
        if on:
            lib.pmx_defer_row_sums(1)
        try:
            yield
        finally:
            if on:
                lib.pmx_defer_row_sums(0)
        rows = lib.pmx_last_partial_rows() if on else 0
        if rows > 0:
            self.pending.append([grad, rows, floats, family, {tuple(sl): False for sl in slices}])

    def claim(self, g):
        """(rows, floats per row) if g is one of the pending slices -- still partial rows, to be summed by the gather -- else (0, 0)."""
        if self.pending and g.dtype == torch.float32 and g.is_contiguous():
            base, key = g.untyped_storage().data_ptr(), (g.storage_offset(), g.numel())
            for buf, rows, floats, _, slices in self.pending:
                if key in slices and buf.untyped_storage().data_ptr() == base:
                    slices[key] = True
                    return rows, floats
        return 0, 0

    def settle(self):
        """After every gradient was offered to `claim`, before the gather is launched: forgets the buffers; raises if a slice is left."""
        pending, self.pending = self.pending, []
        for _, _, _, family, slices in pending:
            for (off, n), claimed in slices.items():
                if not claimed:
                    raise RuntimeError(
                        f"deferred row sums: the {family} gradient at row-0 offset {off} ({n} floats) did not come back from autograd as "
                        "the view its backward returned; a parameter was reached twice in one loss, has a tensor hook, or is no target "
                        "of this call under PPOLearner._backward_group (set PPOLearner.defer_row_sums = False for such a model)")

    def flush(self):
        """Adds whatever partial rows are pending with the dedicated kernel (a consumer other than the learner's gather)."""
        pending, self.pending = self.pending, []
        for buf, rows, floats, _, _ in pending:
            _lib.call("pmx_sum_partial_rows", buf.data_ptr(), rows, floats, _lib.stream(buf.device))


OWNER = _PartialRows()


def buffer(rows, floats, dev):
    """A partial-row gradient buffer [1 + rows][floats] float32, flat: row 0 is the result, the others are the workgroups' parts."""
    return torch.empty((1 + rows) * floats, dtype=torch.float32, device=dev)


def row0(grad, slices, needs):
    """-> (the views of row 0 of a partial-row buffer at `slices`, the slices whose input wants a gradient)."""
    return [grad[o:o + n] for o, n in slices], [sl for sl, need in zip(slices, needs) if need]
