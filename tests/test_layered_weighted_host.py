"""WeightedRCQDecoder(layered=...) host routing (no GPU): "paper" builds engine arguments for the paper's layered schedule
with the decoder's own beta slots and table; every other value keeps the flooding arguments, as the reference does."""
import numpy as np
import pytest

QP = [(3.0, 1.3), (5.0, 1.3), (7.0, 1.3)]


@pytest.mark.parametrize("wtype", [1, 2, 3, 4])
def test_paper_routes_to_layered_schedule_with_beta(wtype):
    import _native as nat
    import codes
    from rcq_decoder import WeightedRCQDecoder
    code = codes.load_code("small_96_48", 10)
    dec = WeightedRCQDecoder(code, 3, 8, QP, weight_sharing_type=wtype, max_iterations=10, layered="paper")
    layout = dec._sharing_layout()
    beta, alpha = dec.weight_tables()
    kw = dec._engine_kwargs(layout, beta, alpha)
    assert kw["schedule"] == nat.SCHED_LAYERED and kw["c2v_form"] == nat.C2V_RCQ
    assert kw["beta"] is beta and np.array_equal(kw["beta_slot"], layout.beta_slot)
    assert kw["beta_slot"].shape == (code.tanner_graph().E,)
    assert np.array_equal(kw["q_of_iter"], [0, 0, 0, 1, 1, 1, 2, 2, 2, 2])


@pytest.mark.parametrize("layered", [False, True, "ref", None])
def test_other_values_keep_flooding(layered):
    import _native as nat
    import codes
    from rcq_decoder import WeightedRCQDecoder
    dec = WeightedRCQDecoder(codes.load_code("small_96_48", 10), 3, 8, QP, weight_sharing_type=2, max_iterations=10,
                             layered=layered)
    kw = dec._engine_kwargs(dec._sharing_layout(), *dec.weight_tables())
    assert kw["schedule"] == nat.SCHED_FLOODING
    assert dec.layered is layered or dec.layered == layered          # stored as given


def test_engine_cache_key_carries_the_schedule():
    import codes
    from rcq_decoder import WeightedRCQDecoder
    dec = WeightedRCQDecoder(codes.load_code("small_96_48", 10), 3, 8, QP, max_iterations=10, layered="paper")
    k_paper = dec._extra_key()
    dec.layered = True
    assert dec._extra_key() != k_paper
