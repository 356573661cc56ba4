"""ctypes binding of libdatok_gpu.so (include/datok_gpu.h).

There is no fallback: if the HIP library is missing or no GPU is usable the
calls raise.  Nothing in this package imports the CPU oracle.
"""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
# DATOK_GPU_LIB selects another build of the same library (A/B timing on one box)
LIB_PATH = os.environ.get("DATOK_GPU_LIB") or os.path.join(_HERE, "libdatok_gpu.so")

# error codes / flags (datok_gpu.h)
OK, E_IO, E_FORMAT, E_NO_DEVICE, E_HIP, E_ARG, E_MODEL, E_CAPACITY, E_STATE, E_NOMEM = 0, -1, -2, -3, -4, -5, -6, -7, -8, -9
E_IRREGULAR = -10
ST_WINDOW_OVERFLOW, ST_EMPTY_TEXT, ST_BAD_MODEL, ST_IRREGULAR, ST_STEP_LIMIT, ST_INTERNAL = 1, 2, 4, 8, 16, 32
ST_BAD_OFFSET = 64

EXPORTS = [
    "dtk_device_count", "dtk_set_device", "dtk_strerror", "dtk_last_hip_error",
    "dtk_model_load", "dtk_model_load_mem", "dtk_model_free", "dtk_model_type", "dtk_model_get_info",
    "dtk_model_info_mem",
    "dtk_batch_create", "dtk_batch_free", "dtk_batch_set_input", "dtk_batch_set_input_device",
    "dtk_batch_run", "dtk_batch_sync", "dtk_batch_stream", "dtk_batch_totals",
    "dtk_batch_set_profiling", "dtk_batch_stage_ms", "dtk_batch_set_chunking", "dtk_batch_set_warm_extend",
    "dtk_batch_result_device", "dtk_batch_result_host", "dtk_transduce", "dtk_free",
    "dtk_foma_to_matok", "dtk_foma_to_datok", "dtk_transduce_replay", "dtk_batch_render_device", "dtk_batch_render_host",
    "dtk_batch_status_host", "dtk_transduce_release", "dtk_transduce_result",
    "dtk_pipeline_create", "dtk_pipeline_free", "dtk_pipeline_set_chunking", "dtk_pipeline_run",
    "dtk_pinned_alloc", "dtk_pinned_free",
    "dtk_batch_set_result_fields", "dtk_batch_download_begin", "dtk_pipeline_set_result_fields",
    "dtk_batch_set_download_stream", "dtk_batch_download_stream", "dtk_batch_done", "dtk_batch_set_streams",
    "dtk_debug_configure", "dtk_batch_debug_stream", "dtk_blk_start", "dtk_blk_end",
    "dtk_multi_create", "dtk_multi_free", "dtk_multi_type", "dtk_multi_set_result_fields", "dtk_multi_set_chunking", "dtk_multi_run",
    "dtk_stream_create", "dtk_stream_free", "dtk_stream_set_chunking", "dtk_stream_set_result_fields", "dtk_stream_run",
    "dtk_stream_transduce", "dtk_stream_set_render",
    "dtk_stream_set_position_render", "dtk_stream_positions", "dtk_stream_emit",
    "dtk_stream_set_offsets", "dtk_stream_offsets", "dtk_blk64_start", "dtk_blk64_end",
    "dtk_batch_sentences_device", "dtk_batch_sentences_host",
    "dtk_stream_set_sentences", "dtk_stream_sentences",
    "dtk_vocab_create", "dtk_vocab_free", "dtk_vocab_size", "dtk_vocab_probe_mem",
    "dtk_tally_create", "dtk_tally_read", "dtk_tally_reset", "dtk_tally_free",
    "dtk_batch_set_vocab", "dtk_batch_token_ids_device", "dtk_batch_token_ids_host",
    "dtk_pipeline_set_vocab", "dtk_stream_set_vocab", "dtk_stream_token_ids",
    "dtk_wordpiece_probe_mem", "dtk_batch_set_wordpiece", "dtk_batch_pieces_device", "dtk_batch_pieces_host",
    "dtk_pipeline_set_wordpiece", "dtk_stream_set_wordpiece", "dtk_stream_pieces",
    "dtk_encode_rows_mem", "dtk_batch_set_encode", "dtk_batch_encoded_device", "dtk_batch_encoded_host",
    "dtk_pipeline_set_encode",
    "dtk_fold_create", "dtk_fold_free", "dtk_fold_apply_mem", "dtk_wordpiece_probe_fold_mem",
    "dtk_batch_set_fold", "dtk_pipeline_set_fold", "dtk_stream_set_fold",
]
ID_UNKNOWN = -1   # DTK_ID_UNKNOWN


class ModelInfo(C.Structure):
    _fields_ = [("kind", C.c_int32), ("epsilon", C.c_int32), ("unknown", C.c_int32),
                ("identity", C.c_int32), ("final_state", C.c_int32), ("sigma_count", C.c_int32),
                ("state_count", C.c_uint32), ("array_len", C.c_uint64),
                ("n_eps_states", C.c_uint32), ("max_eps_chain", C.c_uint32),
                ("entry_bytes", C.c_uint32), ("device_bytes", C.c_uint64),
                ("unknown_used", C.c_uint32), ("dense_states", C.c_uint32),
                ("stream_codes", C.c_uint32), ("lean_walk", C.c_uint32)]


class Totals(C.Structure):
    _fields_ = [("n_docs", C.c_uint32), ("n_bytes", C.c_uint64), ("n_tokens", C.c_uint64),
                ("n_sent", C.c_uint64), ("n_texts", C.c_uint64), ("n_flagged", C.c_uint64),
                ("walk_steps", C.c_uint64), ("n_lanes", C.c_uint32), ("chunk_bytes", C.c_uint32),
                ("repair_rounds", C.c_uint32)]


class ResultView(C.Structure):
    _fields_ = [("tok_off", C.c_void_p), ("sent_off", C.c_void_p), ("text_off", C.c_void_p),
                ("tok_rstart", C.c_void_p), ("tok_rend", C.c_void_p),
                ("tok_bstart", C.c_void_p), ("tok_bend", C.c_void_p),
                ("sent", C.c_void_p), ("text_tok_end", C.c_void_p), ("text_sent_end", C.c_void_p),
                ("status", C.c_void_p), ("ev_bits", C.c_void_p), ("ev_words", C.c_uint64), ("doc_tail", C.c_void_p),
                ("n_exact", C.c_uint32), ("exact_doc", C.c_void_p), ("exact_off", C.c_void_p),
                ("calls", C.c_void_p), ("tok_r16", C.c_void_p),
                ("tok_rblk", C.c_void_p), ("tok_rblk_head", C.c_void_p),
                ("tok_bblk", C.c_void_p), ("tok_bblk_head", C.c_void_p),
                ("evl_off", C.c_void_p), ("evl_pos", C.c_void_p), ("evl_kind", C.c_void_p)]


class SentenceView(C.Structure):
    """dtk_sentence_view: a batch's sentences as rows (dtk_batch_sentences_host / _device)."""
    _fields_ = [("n_sen", C.c_uint64), ("sen_off", C.c_void_p), ("sen_tok_end", C.c_void_p),
                ("sen_bstart", C.c_void_p), ("sen_bend", C.c_void_p), ("sen_rstart", C.c_void_p), ("sen_rend", C.c_void_p),
                ("text_sen_end", C.c_void_p)]


class TokenIdView(C.Structure):
    """dtk_token_id_view: a run's tokens looked up in a vocabulary (dtk_batch_token_ids_host / _device)."""
    _fields_ = [("n_tok", C.c_uint64), ("n_unknown", C.c_uint64), ("tok_id", C.c_void_p)]


class PieceView(C.Structure):
    """dtk_piece_view: a run's tokens split into WordPiece ids (dtk_batch_pieces_host / _device)."""
    _fields_ = [("n_tok", C.c_uint64), ("n_pieces", C.c_uint64), ("n_unknown", C.c_uint64), ("piece_off", C.c_void_p),
                ("piece_id", C.c_void_p), ("piece_bend", C.c_void_p)]


ENC_SENTENCE, ENC_DOCUMENT = 0, 1          # dtk_encode_spec.unit
ENC_FIRST_WINDOW, ENC_WORD_IDS = 1, 2      # dtk_encode_spec.flags


class EncodeSpec(C.Structure):
    """dtk_encode_spec: how sentences or documents become fixed-length model input rows (dtk_batch_set_encode)."""
    _fields_ = [("max_len", C.c_uint32), ("cls_id", C.c_int32), ("sep_id", C.c_int32), ("pad_id", C.c_int32),
                ("unit", C.c_uint32), ("stride", C.c_uint32), ("flags", C.c_uint32)]


class EncodeView(C.Structure):
    """dtk_encode_view: a run's model input rows (dtk_batch_encoded_host / _device)."""
    _fields_ = [("n_units", C.c_uint64), ("n_rows", C.c_uint64), ("n_cut", C.c_uint64), ("max_len", C.c_uint32),
                ("unit_row_off", C.c_void_p), ("input_ids", C.c_void_p), ("row_len", C.c_void_p),
                ("row_piece0", C.c_void_p), ("word_id", C.c_void_p)]


SLICE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p)


class StreamSlice(C.Structure):
    """dtk_stream_slice: one slice of dtk_stream_run (positions relative to the window, whose byte 0 is stream byte base)."""
    _fields_ = [("base", C.c_uint64), ("first", C.c_uint32), ("cut", C.c_uint32), ("len", C.c_uint32),
                ("last", C.c_uint32), ("status", C.c_uint32), ("text", C.c_void_p), ("view", ResultView),
                ("out", C.c_void_p), ("out_len", C.c_uint64)]


class StreamCarry(C.Structure):
    """dtk_stream_carry: the position writer's state at a cut."""
    _fields_ = [("posC", C.c_int64), ("sentB", C.c_uint32), ("init", C.c_uint32), ("pos_nonempty", C.c_uint32),
                ("sent_nonempty", C.c_uint32)]


class StreamPos(C.Structure):
    """dtk_stream_pos: what belongs to a slice's `out` in a position mode (dtk_stream_positions)."""
    _fields_ = [("splice_pos", C.c_uint64), ("splice_sent", C.c_uint64), ("open_pos", C.c_void_p), ("open_pos_len", C.c_uint64),
                ("open_sent", C.c_void_p), ("open_sent_len", C.c_uint64), ("carry_in", StreamCarry), ("carry_out", StreamCarry)]


SO_PLAIN, SO_BLOCKED = 0, 1   # dtk_stream_set_offsets' forms


class StreamOffs(C.Structure):
    """dtk_stream_offs: a slice's rune offsets and sentence list as arrays (dtk_stream_offsets)."""
    _fields_ = [("n_tok", C.c_uint64), ("n_sent", C.c_uint64), ("n_text", C.c_uint64),
                ("tok_rstart", C.c_void_p), ("tok_rend", C.c_void_p), ("tok_rblk", C.c_void_p), ("tok_rblk_head", C.c_void_p),
                ("sent", C.c_void_p), ("text_tok_end", C.c_void_p), ("text_sent_end", C.c_void_p),
                ("carry_in", StreamCarry), ("carry_out", StreamCarry)]


class StreamSenCarry(C.Structure):
    """dtk_stream_sen_carry: the sentence that is open at a cut."""
    _fields_ = [("open", C.c_uint32), ("reserved", C.c_uint32), ("bstart", C.c_uint64), ("bend", C.c_uint64),
                ("rstart", C.c_int64), ("rend", C.c_int64)]


class StreamSens(C.Structure):
    """dtk_stream_sens: the sentences a slice's calls close, as rows (dtk_stream_sentences)."""
    _fields_ = [("n_sen", C.c_uint64), ("n_text", C.c_uint64), ("sen_tok_end", C.c_void_p),
                ("sen_bstart", C.c_void_p), ("sen_bend", C.c_void_p), ("sen_rstart", C.c_void_p), ("sen_rend", C.c_void_p),
                ("text_sen_end", C.c_void_p), ("carry_in", StreamSenCarry), ("carry_out", StreamSenCarry)]


WRITE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t)
READ_FN = C.CFUNCTYPE(C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t)
STREAM_SLICE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(StreamSlice))


class RenderView(C.Structure):
    _fields_ = [("bytes", C.c_void_p), ("doc_off", C.c_void_p), ("total", C.c_uint64)]


class DatokGpuError(RuntimeError):
    def __init__(self, code, what=""):
        L = lib()
        msg = L.dtk_strerror(code).decode()
        if code == E_HIP:
            msg += ": " + L.dtk_last_hip_error().decode()
        super().__init__("%s%s (code %d)" % (what + ": " if what else "", msg, code))
        self.code = code


def build(force=False):
    """Compile libdatok_gpu.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    src_dir = os.path.join(_HERE, "csrc")
    srcs = [os.path.join(src_dir, f) for f in os.listdir(src_dir)
            if f.endswith((".hip", ".cpp", ".h"))]
    srcs += [os.path.join(_HERE, "..", "include", f) for f in ("datok_gpu.h", "datok.hpp")]
    cli = os.path.join(_HERE, "datok")     # the command line (csrc/datok_cli.cpp), built by the same Makefile
    if (not force and os.path.exists(LIB_PATH) and os.path.exists(cli)
            and all(min(os.path.getmtime(LIB_PATH), os.path.getmtime(cli)) >= os.path.getmtime(s) for s in srcs)):
        return LIB_PATH
    subprocess.check_call(["make", "-C", src_dir, "-s"])
    return LIB_PATH


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("datok_amd: %s is missing; run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(there is no CPU fallback)" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    vp, u32, u64, sz = C.c_void_p, C.c_uint32, C.c_uint64, C.c_size_t
    L.dtk_device_count.restype = C.c_int
    L.dtk_set_device.argtypes = [C.c_int]
    L.dtk_strerror.restype = C.c_char_p
    L.dtk_strerror.argtypes = [C.c_int]
    L.dtk_last_hip_error.restype = C.c_char_p
    L.dtk_model_load.argtypes = [C.c_char_p, C.POINTER(vp)]
    L.dtk_model_load_mem.argtypes = [C.c_char_p, sz, C.POINTER(vp)]
    L.dtk_model_free.argtypes = [vp]
    L.dtk_model_free.restype = None
    L.dtk_model_type.restype = C.c_char_p
    L.dtk_model_type.argtypes = [vp]
    L.dtk_model_get_info.argtypes = [vp, C.POINTER(ModelInfo)]
    L.dtk_model_info_mem.argtypes = [C.c_char_p, sz, C.POINTER(ModelInfo)]
    L.dtk_batch_create.argtypes = [u64, u32, C.POINTER(vp)]
    L.dtk_batch_free.argtypes = [vp]
    L.dtk_batch_free.restype = None
    L.dtk_batch_set_input.argtypes = [vp, vp, vp, u32]
    L.dtk_batch_set_input_device.argtypes = [vp, vp, vp, u32, u64]
    L.dtk_batch_run.argtypes = [vp, vp, u32]
    L.dtk_batch_sync.argtypes = [vp]
    L.dtk_batch_stream.restype = vp
    L.dtk_batch_stream.argtypes = [vp]
    L.dtk_batch_totals.argtypes = [vp, C.POINTER(Totals)]
    L.dtk_batch_set_chunking.argtypes = [vp, u32, u32]
    L.dtk_batch_set_warm_extend.argtypes = [vp, u32]
    L.dtk_batch_set_profiling.argtypes = [vp, C.c_int]
    L.dtk_batch_stage_ms.argtypes = [vp, C.POINTER(C.c_float * 9)]
    L.dtk_batch_result_device.argtypes = [vp, C.POINTER(ResultView)]
    L.dtk_batch_result_host.argtypes = [vp, C.POINTER(ResultView)]
    L.dtk_batch_set_result_fields.argtypes = [vp, u32]
    L.dtk_batch_sentences_device.argtypes = [vp, C.POINTER(SentenceView)]
    L.dtk_batch_sentences_host.argtypes = [vp, C.POINTER(SentenceView)]
    L.dtk_sentences_tile_bits.restype = u32      # (no part of the header: where the kernels' tiles end, for the tests)
    L.dtk_batch_download_begin.argtypes = [vp]
    L.dtk_batch_done.argtypes = [vp]
    L.dtk_batch_set_streams.argtypes = [vp, vp, vp]
    L.dtk_batch_set_download_stream.argtypes = [vp, vp]
    L.dtk_batch_download_stream.argtypes = [vp]
    L.dtk_batch_download_stream.restype = vp
    L.dtk_pipeline_set_result_fields.argtypes = [vp, u32]
    L.dtk_transduce.argtypes = [vp, C.c_char_p, sz, u32, C.POINTER(vp), C.POINTER(sz), C.POINTER(u32)]
    L.dtk_transduce_replay.argtypes = L.dtk_transduce.argtypes
    L.dtk_transduce_release.restype = None
    L.dtk_transduce_result.argtypes = [vp, C.c_char_p, sz, u32, C.POINTER(ResultView)]
    L.dtk_batch_render_device.argtypes = [vp, u32, C.POINTER(RenderView)]
    L.dtk_batch_render_host.argtypes = [vp, u32, C.POINTER(RenderView)]
    L.dtk_batch_status_host.argtypes = [vp, vp, u32]
    L.dtk_foma_to_matok.argtypes = [vp, C.c_size_t, C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.dtk_foma_to_matok.restype = C.c_int
    L.dtk_foma_to_datok.argtypes = [vp, C.c_size_t, C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.dtk_foma_to_datok.restype = C.c_int
    L.dtk_free.argtypes = [vp]
    L.dtk_free.restype = None
    L.dtk_pipeline_create.argtypes = [u64, u32, u32, C.POINTER(vp)]
    L.dtk_pipeline_free.argtypes = [vp]
    L.dtk_pipeline_free.restype = None
    L.dtk_pipeline_set_chunking.argtypes = [vp, u32, u32]
    L.dtk_pipeline_run.argtypes = [vp, vp, vp, vp, u32, u32, SLICE_FN, vp]
    L.dtk_multi_create.argtypes = [C.c_char_p, C.POINTER(C.c_int), u32, u64, u32, u32, C.POINTER(vp)]
    L.dtk_multi_free.argtypes = [vp]
    L.dtk_multi_free.restype = None
    L.dtk_multi_type.argtypes = [vp]
    L.dtk_multi_type.restype = C.c_char_p
    L.dtk_multi_set_result_fields.argtypes = [vp, u32]
    L.dtk_multi_set_chunking.argtypes = [vp, u32, u32]
    L.dtk_multi_run.argtypes = [vp, vp, vp, u32, u32, SLICE_FN, vp]
    L.dtk_stream_create.argtypes = [u64, u32, C.POINTER(vp)]
    L.dtk_stream_free.argtypes = [vp]
    L.dtk_stream_free.restype = None
    L.dtk_stream_set_chunking.argtypes = [vp, u32, u32]
    L.dtk_stream_set_result_fields.argtypes = [vp, u32]
    L.dtk_stream_set_render.argtypes = [vp, C.c_int, u32]
    L.dtk_stream_set_position_render.argtypes = [vp, C.c_int, u32]
    L.dtk_stream_positions.argtypes = [vp, C.POINTER(StreamPos)]
    L.dtk_stream_emit.argtypes = [vp, WRITE_FN, vp]
    L.dtk_stream_set_offsets.argtypes = [vp, C.c_int, u32]
    L.dtk_stream_offsets.argtypes = [vp, C.POINTER(StreamOffs)]
    L.dtk_stream_set_sentences.argtypes = [vp, C.c_int]
    L.dtk_stream_sentences.argtypes = [vp, C.POINTER(StreamSens)]
    for f in (L.dtk_blk64_start, L.dtk_blk64_end):
        f.argtypes, f.restype = [vp, vp, u64], C.c_int64
    L.dtk_vocab_create.argtypes = [vp, vp, u32, C.POINTER(vp)]
    L.dtk_vocab_free.argtypes = [vp]
    L.dtk_vocab_free.restype = None
    L.dtk_vocab_size.argtypes = [vp]
    L.dtk_vocab_size.restype = u32
    L.dtk_vocab_probe_mem.argtypes = [vp, vp, u32, vp, sz, C.POINTER(C.c_int32)]
    L.dtk_tally_create.argtypes = [vp, C.POINTER(vp)]
    L.dtk_tally_read.argtypes = [vp, vp]
    L.dtk_tally_reset.argtypes = [vp]
    L.dtk_tally_free.argtypes = [vp]
    L.dtk_tally_free.restype = None
    L.dtk_batch_set_vocab.argtypes = [vp, vp, vp, C.c_int]
    L.dtk_batch_token_ids_device.argtypes = [vp, C.POINTER(TokenIdView)]
    L.dtk_batch_token_ids_host.argtypes = [vp, C.POINTER(TokenIdView)]
    L.dtk_pipeline_set_vocab.argtypes = [vp, vp, vp, C.c_int]
    L.dtk_stream_set_vocab.argtypes = [vp, vp, vp, C.c_int]
    L.dtk_stream_token_ids.argtypes = [vp, C.POINTER(TokenIdView)]
    L.dtk_wordpiece_probe_mem.argtypes = [vp, vp, u32, vp, u32, C.c_int32, u32, vp, sz, vp, vp, u32, C.POINTER(u32)]
    for f in (L.dtk_batch_set_wordpiece, L.dtk_pipeline_set_wordpiece, L.dtk_stream_set_wordpiece):
        f.argtypes = [vp, vp, vp, u32, C.c_int32, u32, C.c_int]
    L.dtk_batch_pieces_device.argtypes = [vp, C.POINTER(PieceView)]
    L.dtk_batch_pieces_host.argtypes = [vp, C.POINTER(PieceView)]
    L.dtk_stream_pieces.argtypes = [vp, C.POINTER(PieceView)]
    L.dtk_fold_create.argtypes = [vp, vp, vp, u32, C.POINTER(vp)]
    L.dtk_fold_free.argtypes = [vp]
    L.dtk_fold_free.restype = None
    L.dtk_fold_apply_mem.argtypes = [vp, vp, vp, u32, vp, sz, vp, sz, C.POINTER(sz)]
    L.dtk_wordpiece_probe_fold_mem.argtypes = [vp, vp, u32, vp, u32, C.c_int32, u32, vp, vp, vp, u32, vp, sz, vp, vp, u32,
                                               C.POINTER(u32)]
    for f in (L.dtk_batch_set_fold, L.dtk_pipeline_set_fold, L.dtk_stream_set_fold):
        f.argtypes = [vp, vp]
    u64 = C.c_uint64
    L.dtk_encode_rows_mem.argtypes = [C.POINTER(EncodeSpec), vp, u64, vp, vp, u64, vp, u32, u64, vp, vp, vp, vp, vp,
                                      C.POINTER(u64), C.POINTER(u64)]
    L.dtk_batch_set_encode.argtypes = [vp, C.POINTER(EncodeSpec), C.c_int]
    L.dtk_pipeline_set_encode.argtypes = [vp, C.POINTER(EncodeSpec), C.c_int]
    L.dtk_batch_encoded_device.argtypes = [vp, C.POINTER(EncodeView)]
    L.dtk_batch_encoded_host.argtypes = [vp, C.POINTER(EncodeView)]
    L.dtk_stream_run.argtypes = [vp, vp, READ_FN, vp, u32, STREAM_SLICE_FN, vp, C.POINTER(u32)]
    L.dtk_stream_transduce.argtypes = [vp, vp, READ_FN, vp, u32, C.POINTER(vp), C.POINTER(sz), C.POINTER(u32)]
    for f in (L.dtk_blk_start, L.dtk_blk_end):
        f.argtypes, f.restype = [vp, vp, u64], C.c_int32
    L.dtk_pinned_alloc.restype = vp
    L.dtk_pinned_alloc.argtypes = [sz]
    L.dtk_pinned_free.argtypes = [vp]
    L.dtk_pinned_free.restype = None
    # Test hooks: the library itself never reads the environment; this harness forwards the DATOK_* switches the tests
    # and scripts set (dtk_debug_configure; unknown names are not the library's and are left alone).
    L.dtk_debug_configure.argtypes = [C.c_char_p, C.c_char_p]
    L.dtk_batch_debug_stream.argtypes = [vp, vp, vp, C.POINTER(u32)]
    for k, v in os.environ.items():
        if k.startswith("DATOK_") and k not in ("DATOK_GPU_LIB", "DATOK_GATHER_TIMEOUT"):
            L.dtk_debug_configure(k.encode(), v.encode())
    _lib = L
    return L


def check(code, what=""):
    if code != OK:
        raise DatokGpuError(code, what)
