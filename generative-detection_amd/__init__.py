"""MI355X-native OD-VAE autoencoder training path (host side).  Import it as `odvae_amd`."""
__version__ = "0.1.0"


def set_float32_matmul_precision(name):
    """highest (default) | high | medium | torch: how exactly the f32 products of the attention (and the 1x1 convolutions' deep weight
    gradient) are formed on the bf16 matrix pipe; ops/precision.py.  The op layer is imported on first use."""
    from . import ops
    ops.set_float32_matmul_precision(name)


def get_float32_matmul_precision():
    from . import ops
    return ops.get_float32_matmul_precision()
