"""The structs of the layer-wise path's C ABI, filled for the tests that call its entry points directly (include/distr_train.h). The
Python layer itself describes every network as distr_train_net (functions._train_net_struct); the calls that take
distr_train_weights stay in the ABI, and these tests are their callers."""


def _address(t):
    return t.data_ptr() if hasattr(t, 'data_ptr') else int(t)


def train_weights(weights, latent_size):
    """distr_train_weights of code length `latent_size` on weights = [W0..W8, b0..b8]: device tensors, or plain addresses"""
    from distr import binding
    tw = binding.TrainWeights(latent_size=int(latent_size))
    for l in range(9):
        tw.W[l] = _address(weights[l])
        tw.b[l] = _address(weights[9 + l])
    return tw


def train_grads(grads):
    """distr_train_grads on grads = [g_W0..g_W8, g_b0..g_b8]: device tensors, or plain addresses"""
    from distr import binding
    tg = binding.TrainGrads()
    for l in range(9):
        tg.g_W[l] = _address(grads[l])
        tg.g_b[l] = _address(grads[9 + l])
    return tg
