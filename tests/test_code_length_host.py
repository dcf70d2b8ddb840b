"""Host side of decoders with a code length C other than 256: shape validation, packing, the fixture generator."""
import numpy as np
import pytest

from distr import decoder_pack, fixture

F1_SHA256 = '9a909d90efaf677e85a4283115e6a3479508a6d0d1d8e2c9ff47062fc3318858'


def test_default_fixture_unchanged():
    Ws, bs, latent = fixture.make_decoder_weights()
    assert fixture.weights_sha256(Ws, bs) == F1_SHA256
    assert latent.shape == (1, 256)
    Ws2, bs2, latent2 = fixture.make_decoder_weights(latent_size=256)
    assert fixture.weights_sha256(Ws2, bs2) == F1_SHA256 and np.array_equal(latent, latent2)


@pytest.mark.parametrize('C', [1, 64, 128, 255, 256, 300, 400, 508])
def test_validate_and_flatten_accepts(C):
    Ws, bs, latent = fixture.make_decoder_weights(latent_size=C)
    assert [W.shape for W in Ws] == fixture.layer_shapes(C) and latent.shape == (1, C)
    assert Ws[3].shape == (509 - C, 512) and Ws[4].shape == (512, 512)
    assert decoder_pack.validate(Ws, bs) == C
    flat = decoder_pack.flatten(Ws, bs)
    assert flat.dtype == np.float32 and flat.size == sum(W.size + b.size for W, b in zip(Ws, bs))
    assert decoder_pack.latent_size_of(Ws) == C


def test_bad_shapes_refused():
    Ws, bs, _ = fixture.make_decoder_weights(latent_size=300)
    for C in (0, 509):                        # lin0's width gives the code length: 0 and 509 are outside 1..508
        bad = [W.copy() for W in Ws]
        bad[0] = np.zeros((512, C + 3), np.float32)
        with pytest.raises(decoder_pack.UnsupportedDecoder, match='outside 1..508'):
            decoder_pack.flatten(bad, bs)
    bad = [W.copy() for W in Ws]
    bad[3] = np.zeros((253, 512), np.float32)            # lin3 of the C = 256 decoder with a C = 300 lin0
    with pytest.raises(decoder_pack.UnsupportedDecoder, match='lin3'):
        decoder_pack.flatten(bad, bs)
    bad = [W.copy() for W in Ws]
    bad[4] = np.zeros((512, 511), np.float32)
    with pytest.raises(decoder_pack.UnsupportedDecoder, match='lin4'):
        decoder_pack.flatten(bad, bs)
    badb = [b.copy() for b in bs]
    badb[3] = np.zeros(253, np.float32)
    with pytest.raises(decoder_pack.UnsupportedDecoder, match='lin3'):
        decoder_pack.flatten(Ws, badb)


def test_fixture_has_a_surface():
    """The fixture decoder of every tested code length has its zero level set inside the unit sphere: negative at the origin,
    positive on the sphere (float64 evaluation of the decoder)."""
    rs = np.random.RandomState(0)
    d = rs.standard_normal((500, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    pts = np.concatenate([np.zeros((1, 3)), d])
    for C in (1, 64, 128, 256, 300, 508):
        Ws, bs, latent = fixture.make_decoder_weights(latent_size=C)
        inp = np.concatenate([np.repeat(latent.astype(np.float64), len(pts), 0), pts], 1)
        x = inp
        for l in range(9):
            if l == 4:
                x = np.concatenate([x, inp], 1)
            x = x @ Ws[l].T.astype(np.float64) + bs[l]
            if l < 8:
                x = np.maximum(x, 0.0)
        f = np.tanh(x[:, 0])
        assert f[0] < 0 and f[1:].min() > 0, (C, f[0], f[1:].min())
