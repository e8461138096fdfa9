"""-m gpu: every call form INTERLEAVED on one handle. The bit tests of the single forms (test_gpu_fullsize, test_gpu_corpus,
test_gpu_pairs) hold fused ≡ separate for one form at a time; what one call leaves behind for the next — a request that outlives
its call, a stream that was to be followed, a decay queued with another step's learning rate — only shows when the forms follow
each other. Handle A runs tests/step_requests.SEQUENCE through the fused entry points, handle B (same seed, same inputs) as
compute_cost*; compute_gradients; update; both get the two refused calls. After EVERY call the parameters, the optimiser state and
the cost are equal bit for bit — nothing here has a tolerance: the two forms run the same kernels on the same data in the same
order per buffer."""
import numpy as np
import pytest

from tests.step_requests import FUSED_TEXT_STEPS, Inputs, call
from tests.test_gpu_corpus import assert_same_state

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape", ["a", "b"])
def test_interleaved_call_forms_fused_equal_separate(shape):
    inp = Inputs(shape)
    A, B = inp.model(), inp.model()
    if shape == "a":
        A.profile_enable(True)
    for i, (kind, x) in enumerate(inp.calls):
        ra, rb = call(A, kind, x, inp.lr, True), call(B, kind, x, inp.lr, False)
        what = "call %d (%s)" % (i, kind)
        if kind in ("no_corpus", "bad_lr"):
            assert ra == 1 and rb == 1, what                    # NVSM_ERR_INVALID_ARGUMENT from both forms
        else:
            assert np.isfinite(ra) and np.float32(ra).view(np.uint32) == np.float32(rb).view(np.uint32), (what, ra, rb)
        if kind == "no_corpus":
            A.upload_corpus(inp.corpus)
            B.upload_corpus(inp.corpus)
        else:
            assert A.get_cost() == B.get_cost(), what           # (also behind the refused step: its forward pass stands)
        assert_same_state(A, B)
    for m in (A, B):
        assert not m.get_tensor("arrival_counters").any()
    if shape == "a":
        # the paths this shape is chosen for, once per fused step with a text objective (the refused step stops in front of them):
        # 20 000 word rows against 2 560 entries split the words pass (row_pass_split), lambda > 0 and SGD hoist the decay of the
        # rows without entries behind the CSR build, and the dT product's slabs are added up by the projection update
        notes = A.profile()
        assert notes.get("untouched_words_hoisted", (0.0, 0))[1] == FUSED_TEXT_STEPS, notes
        assert notes.get("slab_sum_in_update", (0.0, 0))[1] == FUSED_TEXT_STEPS, notes
