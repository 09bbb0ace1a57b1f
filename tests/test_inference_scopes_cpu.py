"""CPU: the two scopes the inference paths share -- the decoder's inference modes (model._ProjHolder.inference) and the
Monte-Carlo sampling state (model.mc_sampling) -- set what they say, put back exactly what they found on a normal exit and on
an exception, and refuse nesting, grad mode and a model with nothing to sample.  Attributes only: nothing here launches."""
import pytest
import torch

from bayeslms_amd import model as M
from bayeslms_amd._lib import BayesLMError


def _modes(dec):
    return dec.rows, dec.nll_targets, dec.return_input


def test_decoder_scope_sets_and_restores():
    dec = M._ProjHolder(8, 12)
    rows, tgt = torch.tensor([2, 0]), torch.tensor([1, 5])
    assert _modes(dec) == (None, None, False)
    with torch.no_grad():
        with dec.inference(rows=rows, targets=tgt) as d:
            assert d is dec and dec.rows is rows and dec.nll_targets is tgt and dec.return_input is False
            other = torch.tensor([3, 4])
            dec.set_nll_targets(other)  # new targets without leaving the scope (engine.evaluate, per window)
            assert dec.nll_targets is other and dec.rows is rows
        assert _modes(dec) == (None, None, False)
        with dec.inference(input_rows=True):
            assert _modes(dec) == (None, None, True)
        assert _modes(dec) == (None, None, False)


def test_decoder_scope_restores_after_an_exception_and_can_be_entered_again():
    dec = M._ProjHolder(8, 12)
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="inside"):
            with dec.inference(rows=torch.tensor([1]), input_rows=True):
                raise RuntimeError("inside")
        assert _modes(dec) == (None, None, False)
        with dec.inference(input_rows=True):  # the failed scope did not leave the decoder locked
            pass
        assert _modes(dec) == (None, None, False)


def test_decoder_scope_hands_back_selected_input_rows_then_the_logits_path_again():
    dec = M._ProjHolder(8, 12)
    x = torch.arange(3 * 2 * 8, dtype=torch.float32).view(3, 2, 8)
    rows = torch.tensor([4, 1])
    with torch.no_grad(), dec.inference(rows=rows, input_rows=True):
        got = dec(x)
    assert torch.equal(got, x.reshape(6, 8)[rows])
    assert _modes(dec) == (None, None, False)  # decoder(x) is on the logits path again


def test_decoder_scope_refuses_nesting_and_grad_mode():
    dec, other = M._ProjHolder(8, 12), M._ProjHolder(8, 12)
    with torch.no_grad(), dec.inference(input_rows=True):
        with pytest.raises(BayesLMError, match="does not nest"):
            with dec.inference(targets=torch.tensor([0])):
                pass
        assert _modes(dec) == (None, None, True)  # the refused entry changed nothing
        with other.inference(input_rows=True):  # another decoder (two-model scoring) has its own scope
            pass
    with pytest.raises(BayesLMError, match="inference-only"):
        with dec.inference(input_rows=True):
            pass
    assert _modes(dec) == (None, None, False)
    with pytest.raises(BayesLMError, match="no inference scope"):
        dec.set_nll_targets(torch.tensor([0]))
    with torch.no_grad(), dec.inference(input_rows=True):
        with torch.enable_grad(), pytest.raises(BayesLMError, match="inference-only"):
            dec(torch.zeros(2, 8))  # grad mode switched back on inside the scope: forward still refuses


def _gauss_transformer():
    return M.GaussTransformerModel(50, 16, 2, 32, 2, 0.5, True, 3).eval()


def _state(m):
    ns = m.noise_state
    return ns.seed, ns.step, ns.auto_step


@pytest.mark.parametrize("fail", [False, True])
def test_mc_sampling_state_and_restore(fail):
    m = _gauss_transformer()
    m.set_seed(77)
    m.noise_state.step = 5  # auto_step stays True: nobody has taken the counter over
    before = _state(m)
    assert before == (77, 5, True)
    lowered = [s for s in M.variational_sites(m) if getattr(s, "sample", True) is False]
    assert lowered  # the GPNN flags are down by default: the scope has something to raise
    try:
        with M.mc_sampling(m, 4321, 3):
            assert m.training and m.noise_state.dropout_off is True and m.noise_state.seed == 4321
            assert all(s.sample is True for s in lowered)
            assert all(s.training for s in M.variational_sites(m))
            m.set_step(2)
            assert (m.noise_state.step, m.noise_state.auto_step) == (2, False)
            if fail:
                raise KeyError("inside")
    except KeyError:
        assert fail
    assert m.training is False and not any(s.training for s in m.modules())
    assert m.noise_state.dropout_off is False
    assert all(s.sample is False for s in lowered)
    assert _state(m) == before


def test_mc_sampling_leaves_flags_that_were_already_up():
    m = M.BayesTransformerModel(50, 16, 2, 32, 2, 0.5, True, "FFN").eval()
    sites = M.variational_sites(m)
    assert sites and all(s.sample is True for s in sites)
    with M.mc_sampling(m, 1, 2):
        pass
    assert all(s.sample is True for s in sites) and m.training is False


def test_mc_sampling_refuses_a_model_without_variational_sites():
    m = M.TransformerModel(50, 16, 2, 32, 2, 0.5, "gelu", True).eval()
    before = _state(m)
    msg = r"--mc-samples 4: TransformerModel has no variational tensor to sample \(mean-weight scoring is --mc-samples 0\)"
    with pytest.raises(BayesLMError, match=msg):
        with M.mc_sampling(m, 1111, 4):
            pass
    with pytest.raises(BayesLMError, match=msg):
        M.require_variational_sites(m, 4)
    assert m.training is False and m.noise_state.dropout_off is False and _state(m) == before
