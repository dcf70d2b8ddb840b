"""decoder_pack.validate refuses non-finite weights: the compacted 64-ray tile skips products with +0, which equals the full chain only
when no weight is inf / nan."""
import numpy as np
import pytest


@pytest.mark.parametrize('bad', [np.inf, -np.inf, np.nan])
@pytest.mark.parametrize('where', ['weight', 'bias'])
def test_non_finite_weights_are_refused(bad, where):
    from distr import decoder_pack, fixture
    Ws, bs, _ = fixture.make_decoder_weights()
    decoder_pack.validate(Ws, bs)
    Ws, bs = [W.copy() for W in Ws], [b.copy() for b in bs]
    if where == 'weight':
        Ws[5][17, 300] = bad
    else:
        bs[2][511] = bad
    with pytest.raises(decoder_pack.UnsupportedDecoder, match='non-finite'):
        decoder_pack.flatten(Ws, bs)
