"""ctcext_amd — MI355X-native CTC beam search with per-beam best-alignment
tracking; a drop-in for prouast/ctc-beam-search-op's
``ctc_ext_beam_search_decoder`` (tensorflow_ctc_ext_beam_search_decoder/__init__.py:19).
"""
from .ops import (CTCExtBeamSearchDecoder, Decoder, DenseDecode, FailedPreconditionError, InternalError,
                  InvalidArgumentError, OpError, StablePrefix, StreamDecoder, StreamDense, TokenScores, TokenTimes,
                  UnimplementedError, ctc_ext_beam_search_decoder, decode_dense, decode_logits, dense_check,
                  dense_path_scores, dense_token_scores, dense_token_times, get_decoder, kept_frames, path_score_row,
                  path_scores, token_scores, token_scores_row, token_times, token_times_row,
                  PathAlignments, dense_path_alignments, path_alignments, path_alignment_row,
                  decode_greedy, greedy_row, GreedyPush, GreedyStream, dense_target_scores, score_targets,
                  TargetAlignments, dense_target_alignments, forced_align, dense_transcript_alignments,
                  align_transcripts, dense_prefix_scores, score_prefixes, prefix_score_row,
                  TargetGrads, dense_target_grads, target_grads, score_targets_autograd, target_grad_row)

__all__ = ["ctc_ext_beam_search_decoder", "decode_logits", "CTCExtBeamSearchDecoder", "Decoder", "get_decoder", "StreamDecoder",
           "StablePrefix", "StreamDense",
           "decode_dense", "dense_check", "DenseDecode",
           "dense_token_times", "token_times", "token_times_row", "TokenTimes", "kept_frames",
           "dense_token_scores", "token_scores", "token_scores_row", "TokenScores",
           "dense_path_scores", "path_scores", "path_score_row",
           "dense_path_alignments", "path_alignments", "path_alignment_row", "PathAlignments",
           "decode_greedy", "greedy_row", "GreedyStream", "GreedyPush",
           "dense_target_scores", "score_targets",
           "dense_target_alignments", "forced_align", "TargetAlignments",
           "dense_transcript_alignments", "align_transcripts",
           "dense_prefix_scores", "score_prefixes", "prefix_score_row",
           "dense_target_grads", "target_grads", "score_targets_autograd", "target_grad_row", "TargetGrads",
           "OpError", "InvalidArgumentError", "FailedPreconditionError", "UnimplementedError",
           "InternalError"]
