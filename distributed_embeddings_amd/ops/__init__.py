from .embedding_lookup import (Ragged, dequantize_rowwise_int4,
                               dequantize_rowwise_int8, deterministic,
                               embedding_lookup, is_deterministic,
                               multi_hot_expand, quantize_rowwise_int4,
                               quantize_rowwise_int8,
                               quantized_embedding_lookup, row_to_split,
                               set_deterministic, stochastic_round_bf16)
