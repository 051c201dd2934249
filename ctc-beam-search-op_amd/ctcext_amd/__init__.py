"""ctcext_amd — MI355X-native CTC beam search with per-beam best-alignment
tracking; a drop-in for prouast/ctc-beam-search-op's
``ctc_ext_beam_search_decoder`` (tensorflow_ctc_ext_beam_search_decoder/__init__.py:19).
"""
from .ops import (CTCExtBeamSearchDecoder, Decoder, DenseDecode, FailedPreconditionError, InternalError,
                  InvalidArgumentError, OpError, StablePrefix, StreamDecoder, StreamDense, TokenScores, TokenTimes,
                  UnimplementedError, ctc_ext_beam_search_decoder, decode_dense, decode_logits, dense_check,
                  dense_token_scores, dense_token_times, get_decoder, kept_frames, token_scores, token_scores_row,
                  token_times, token_times_row)

__all__ = ["ctc_ext_beam_search_decoder", "decode_logits", "CTCExtBeamSearchDecoder", "Decoder", "get_decoder", "StreamDecoder",
           "StablePrefix", "StreamDense",
           "decode_dense", "dense_check", "DenseDecode",
           "dense_token_times", "token_times", "token_times_row", "TokenTimes", "kept_frames",
           "dense_token_scores", "token_scores", "token_scores_row", "TokenScores",
           "OpError", "InvalidArgumentError", "FailedPreconditionError", "UnimplementedError",
           "InternalError"]
