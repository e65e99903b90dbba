"""Parts of the Centaur text-to-speech family."""
from .attention import padding_bias, wide_attention

__all__ = ["padding_bias", "wide_attention"]
