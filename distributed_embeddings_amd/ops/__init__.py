from .embedding_lookup import (Ragged, dequantize_rowwise_int4,
                               dequantize_rowwise_int8, embedding_lookup,
                               quantize_rowwise_int4, quantize_rowwise_int8,
                               quantized_embedding_lookup, row_to_split,
                               stochastic_round_bf16)
