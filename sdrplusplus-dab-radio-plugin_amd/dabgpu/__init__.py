"""Thin ctypes binding of libdabgpu.so (the C ABI in include/dabgpu.h).

Plumbing only: argument marshalling and error translation.  There is no Python or
CPU implementation behind these calls -- if the HIP library is missing or no gfx950
device is visible they raise.  Used by tests/, bench.py and __graft_entry__.py.
"""
import atexit
import ctypes as C
import os
import sys
import weakref

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DABGPU_LIB", os.path.join(os.path.dirname(_HERE), "libdabgpu.so"))

NB_FFT = 2048
NB_CP = 504
NB_SYM = 2552
NB_NULL = 2656
NB_SYMBOLS = 76
NB_CARRIERS = 1536
NB_FRAME_BITS = 230400
NB_FRAME_SAMPLES = 196608
NB_FIC_BITS = 9216
NB_CIF_BITS = 55296
FRAME_USED_SAMPLES = NB_SYMBOLS * NB_SYM

#: every symbol include/dabgpu.h declares (tests check the library exports all of them)
EXPORTS = [
    "dabgpu_abi_version", "dabgpu_strerror", "dabgpu_get_ofdm_params", "dabgpu_get_dab_params",
    "dabgpu_get_prs_reference", "dabgpu_get_mapper_reference", "dabgpu_create", "dabgpu_destroy",
    "dabgpu_sync", "dabgpu_stream", "dabgpu_ofdm_demod_frames_dev", "dabgpu_ofdm_demod_frames",
    "dabgpu_fft_symbols_dev", "dabgpu_fft_symbols", "dabgpu_fic_decode_dev", "dabgpu_fic_decode",
    "dabgpu_subchannel_bytes", "dabgpu_msc_decode_dev", "dabgpu_msc_decode", "dabgpu_viterbi_dev",
    "dabgpu_viterbi", "dabgpu_set_timing", "dabgpu_last_kernel_ms", "dabgpu_sync_prs_dev", "dabgpu_sync_prs",
    "dabgpu_msc_decode_multi_dev", "dabgpu_dabplus_superframes_dev", "dabgpu_dabplus_superframes",
    "dabgpu_acquire_default_cfg", "dabgpu_acquire_dev", "dabgpu_acquire", "dabgpu_ofdm_demod_acquired_dev",
    "dabgpu_ofdm_set_soft_selection", "dabgpu_soft_selection", "dabgpu_uep_subchannel",
    "dabgpu_host_alloc", "dabgpu_host_free", "dabgpu_decode_frames_dev", "dabgpu_decode_frames",
    "dabgpu_streams_reset", "dabgpu_stream_states", "dabgpu_set_stream_offsets", "dabgpu_ofdm_demod_streams_dev",
    "dabgpu_ofdm_demod_streams", "dabgpu_get_stats", "dabgpu_mean_kernel_ms", "dabgpu_decode_stream_frames",
    "dabgpu_decode_stream_reset", "dabgpu_alloc_frame_buffers", "dabgpu_free_frame_buffers",
    "dabgpu_mover_frames_dev", "dabgpu_pipe_open", "dabgpu_pipe_submit", "dabgpu_pipe_wait", "dabgpu_pipe_reset", "dabgpu_pipe_close",
    "dabgpu_set_stream_loop", "dabgpu_set_loop_gate", "dabgpu_track_default_cfg", "dabgpu_track_start_dev", "dabgpu_ofdm_demod_tracked_dev",
    "dabgpu_ofdm_demod_stream_frame", "dabgpu_ofdm_demod_frames_dd_dev", "dabgpu_test_fail_frame_call",
    "dabgpu_mer_dev", "dabgpu_channel_ber_dev", "dabgpu_decode_stream_frames_quality",
    "dabgpu_set_iq_format", "dabgpu_get_iq_format",
    "dabgpu_tii_default_cfg", "dabgpu_tii_pattern", "dabgpu_tii_frames_dev", "dabgpu_tii_acquired_dev", "dabgpu_tii_decode",
    "dabgpu_cir_default_cfg", "dabgpu_cir_frames_dev", "dabgpu_cir_acquired_dev", "dabgpu_cir_analyse",
    "dabgpu_eti_layout", "dabgpu_eti_history_bytes", "dabgpu_eti_frames_dev", "dabgpu_eti_parse",
    "dabgpu_eti_streams_from_frame", "dabgpu_mod_default_cfg", "dabgpu_mod_state_bytes", "dabgpu_modulate_eti_dev",
    "dabgpu_decode_ensembles_dev", "dabgpu_fig_subchannels",
    "dabgpu_dabplus_follow_dev", "dabgpu_dabplus_carry_bytes", "dabgpu_fig_audio_components",
    "dabgpu_pad_state_bytes", "dabgpu_pad_labels_dev", "dabgpu_pad_labels_host", "dabgpu_pad_label_utf8",
    "dabgpu_mp2_carry_bytes", "dabgpu_mp2_follow_dev", "dabgpu_mp2_follow_host",
    "dabgpu_mp2_subbands_dev", "dabgpu_mp2_subbands_host",
    "dabgpu_mot_state_bytes", "dabgpu_mot_arena_bytes", "dabgpu_mot_slides_dev", "dabgpu_mot_slides_host", "dabgpu_mot_header_parse",
    "dabgpu_fig_packet_components", "dabgpu_packet_state_bytes", "dabgpu_packet_slides_dev", "dabgpu_packet_slides_host",
    "dabgpu_packet_fec_state_bytes", "dabgpu_packet_fec_delay", "dabgpu_packet_fec_dev", "dabgpu_packet_fec_host",
    "dabgpu_packet_fec_erasures_dev", "dabgpu_packet_fec_erasures_host",
    "dabgpu_packet_carousel_state_bytes", "dabgpu_packet_carousel_arena_bytes", "dabgpu_packet_carousel_dev",
    "dabgpu_packet_carousel_host", "dabgpu_mot_directory_parse",
    "dabgpu_packet_groups_state_bytes", "dabgpu_packet_groups_chunk", "dabgpu_packet_groups_dev", "dabgpu_packet_groups_host",
    "dabgpu_fig_user_applications",
    "dabgpu_eti_read_state_bytes", "dabgpu_eti_read_dev", "dabgpu_eti_read_host",
    "dabgpu_edi_packet_bytes", "dabgpu_edi_frames_dev", "dabgpu_edi_parse", "dabgpu_edi_streams_from_packet",
    "dabgpu_edi_read_state_bytes", "dabgpu_edi_read_max_rows", "dabgpu_edi_read_dev", "dabgpu_edi_read_host",
    "dabgpu_pft_layout", "dabgpu_pft_fragments_dev", "dabgpu_pft_fragments_host", "dabgpu_pft_read_state_bytes",
    "dabgpu_pft_read_out_bytes", "dabgpu_pft_read_max_records", "dabgpu_pft_read_dev", "dabgpu_pft_read_host",
    "dabgpu_dmb_state_bytes", "dabgpu_dmb_max_packets", "dabgpu_dmb_state_census", "dabgpu_dmb_follow_dev", "dabgpu_dmb_follow_host",
    "dabgpu_fig_stream_components", "dabgpu_ts_programs",
]

ABI_VERSION = 6
PLACE_PLAIN, PLACE_DOMAINS = 0, 1
PLAIN_ONE_DOMAIN = 7
PLAIN_REASONS = {0: "plain requested", 1: "buffers too small (or too many chunks) for placement", 2: "virtual-memory API refused",
                 3: "no room for the chunks", 4: "the context's domain-aware pair is still alive",
                 5: "larger than the context's reserved address range", 6: "probe launch failed",
                 7: "the placed pair's own check read >= 0.985 (one HBM domain behind the virtual-memory API on this box): "
                    "given back, two plain allocations made instead"}
FLAG_VITERBI_WAVE = 1 << 0
FLAG_VITERBI_LANE = 1 << 1
FLAG_LANE_UNFUSED = 1 << 2
FLAG_TEST_ONE_DOMAIN = 1 << 30          # test hook: the allocator's check of a placed pair reads 1.00
#: sample formats of the device-pointer calls and the ring (Context.set_iq_format); cu8's value is u - 127.5
IQ_CF32, IQ_CS16, IQ_CS8, IQ_CU8 = 0, 1, 2, 3
#: numpy dtype of one I or Q value per format
IQ_DTYPES = {IQ_CF32: np.dtype(np.float32), IQ_CS16: np.dtype(np.int16), IQ_CS8: np.dtype(np.int8), IQ_CU8: np.dtype(np.uint8)}


class DabGpuError(RuntimeError):
    def __init__(self, status, what):
        self.status = status
        super().__init__("%s failed: %s (%d)" % (what, strerror(status), status))


class OfdmParams(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "nb_frame_symbols", "nb_symbol_period", "nb_null_period", "nb_fft", "nb_cyclic_prefix",
        "nb_data_carriers", "freq_carrier_spacing", "nb_frame_samples")]


class DabParams(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "nb_frame_bits", "nb_symbols", "nb_fic_symbols", "nb_msc_symbols", "nb_sym_bits", "nb_fic_bits",
        "nb_msc_bits", "nb_fibs", "nb_cifs", "nb_fib_bits", "nb_fib_cif_bits", "nb_fibs_per_cif",
        "nb_cif_bits")]


class Cfg(C.Structure):
    _fields_ = [("device", C.c_int32), ("max_frames", C.c_int32), ("transmission_mode", C.c_int32),
                ("flags", C.c_int32), ("ofdm_symbol_runs", C.c_int32), ("reserved", C.c_int32 * 3)]


class Stats(C.Structure):
    _fields_ = [("state", C.c_int32), ("fine_freq_offset", C.c_float), ("coarse_freq_offset", C.c_float),
                ("net_freq_offset", C.c_float), ("signal_average", C.c_float), ("total_frames_read", C.c_int32),
                ("total_frames_desync", C.c_int32), ("last_fine_error", C.c_float), ("tracking", C.c_int32),
                ("last_time_offset", C.c_int32), ("next_frame_start", C.c_double), ("drift", C.c_float),
                ("last_peak_to_mean", C.c_float), ("loop_gated", C.c_int32), ("reserved", C.c_int32)]


STREAM_STATE_DTYPE = np.dtype([("fine_freq_offset", np.float32), ("coarse_freq_offset", np.float32),
                               ("signal_average", np.float32), ("last_fine_error", np.float32),
                               ("total_frames_read", np.int32), ("total_frames_desync", np.int32),
                               ("tracking", np.int32), ("last_time_offset", np.int32),
                               ("next_frame_start", np.float64), ("drift", np.float32), ("last_peak_to_mean", np.float32),
                               ("loop_gated", np.int32), ("dd_branch", np.int32), ("dd_pending", np.int32),
                               ("reserved", np.int32)])     # 64 bytes, device-resident
assert STREAM_STATE_DTYPE.itemsize == 64

# reception quality (include/dabgpu.h: dabgpu_mer per frame, dabgpu_ber_count per codeword)
MER_DTYPE = np.dtype([("signal", np.uint64), ("error", np.uint64), ("carriers", np.int32), ("reserved", np.int32)])
assert MER_DTYPE.itemsize == 24
BER_DTYPE = np.dtype([("errors", np.uint32), ("bits", np.uint32)])
assert BER_DTYPE.itemsize == 8
#: dabgpu_superframe_status: one DAB+ super-frame's checks (include/dabgpu.h)
SUPERFRAME_STATUS_DTYPE = np.dtype([("firecode_ok", np.int32), ("rs_corrected", np.int32), ("rs_uncorrectable", np.int32),
                                    ("num_aus", np.int32), ("au_crc_mask", np.int32), ("au_start", np.int32, (8,)),
                                    ("reserved", np.int32, (3,))])
assert SUPERFRAME_STATUS_DTYPE.itemsize == 64
#: dabgpu_dabplus_follow_result: what one entry of Context.dabplus_follow_dev did in one call (device memory)
DABPLUS_FOLLOW_RESULT_DTYPE = np.dtype([("n_superframes", np.int32), ("phase", np.int32), ("synced", np.int32),
                                        ("dropped", np.int32), ("raw_hits", np.int32), ("held", np.int32),
                                        ("reserved", np.int32, (2,))])
assert DABPLUS_FOLLOW_RESULT_DTYPE.itemsize == 32
#: dabgpu_pad_label: the dynamic label of one followed DAB+ service (text bytes behind `length` are zero)
PAD_LABEL_DTYPE = np.dtype([("length", np.int32), ("charset", np.int32), ("toggle", np.int32), ("reserved", np.int32),
                            ("text", np.uint8, (128,))])
assert PAD_LABEL_DTYPE.itemsize == 144
#: dabgpu_pad_result: what one entry of pad_labels_dev / pad_labels_host counted in one call
PAD_RESULT_DTYPE = np.dtype([(n, np.int32) for n in (
    "aus", "aus_lost", "aus_with_xpad", "pad_malformed", "fields_ignored", "groups_ok", "groups_crc_failed",
    "commands_ignored", "labels_completed", "changes")] + [("reserved", np.int32, (6,))])
assert PAD_RESULT_DTYPE.itemsize == 64
PAD_CHARSET_EBU_LATIN, PAD_CHARSET_UCS2, PAD_CHARSET_UTF8 = 0, 6, 15
#: dabgpu_mp2_result: what one entry of Context.mp2_follow_dev / mp2_follow_host found and counted in one call
MP2_RESULT_DTYPE = np.dtype([(n, np.int32) for n in (
    "id", "sample_rate", "bitrate_kbps", "mode", "phase", "held", "synced", "hits", "frames", "header_errors", "crc_failed",
    "frames_no_crc", "dropped")] + [("reserved", np.int32, (3,))])
assert MP2_RESULT_DTYPE.itemsize == 64
#: a row of the layer-II follow call, and the bit rate the PAD / slideshow entries name for such rows (110 * 16 / 8 = 220)
MP2_ROW_BYTES, MP2_PAD_KBPS = 220, 16
#: dabgpu_mp2_level: the audio level record of one row of Context.mp2_subbands_dev / mp2_subbands_host (sub-band domain)
MP2_LEVEL_DTYPE = np.dtype([("kind", np.int32), ("channels", np.int32), ("cells", np.int32), ("scf63", np.int32),
                            ("power", np.float32, (2,)), ("peak", np.float32, (2,))])
assert MP2_LEVEL_DTYPE.itemsize == 32
MP2_AUDIO_DECODED, MP2_AUDIO_NOT_GOOD, MP2_AUDIO_OVERRUN = 0, 1, 2
#: dabgpu_mp2_audio_result: the rows of one entry in one call by kind, and the decoded ones whose power is zero
MP2_AUDIO_RESULT_DTYPE = np.dtype([(n, np.int32) for n in ("decoded", "not_good", "overrun", "silent")] + [("reserved", np.int32, (4,))])
assert MP2_AUDIO_RESULT_DTYPE.itemsize == 32
#: the sub-band samples of one row: [channel][sample][sub-band] float32
MP2_SUBBANDS_SHAPE = (2, 36, 32)
#: dabgpu_mot_slide: the record in front of every slide in its slot (then header_bytes of MOT header, then body_bytes of body)
MOT_SLIDE_DTYPE = np.dtype([(n, np.int32) for n in (
    "transport_id", "content_type", "content_subtype", "header_bytes", "body_bytes", "superframe", "au", "reserved")])
assert MOT_SLIDE_DTYPE.itemsize == 32
#: dabgpu_mot_result: what one entry of mot_slides_dev / mot_slides_host counted in one call
MOT_COUNTERS = ("aus", "aus_lost", "aus_with_xpad", "pad_malformed", "fields_ignored", "lengths_ok", "lengths_ignored", "groups_no_length",
                "groups_ok", "groups_crc_failed", "groups_ignored_type", "groups_no_transport_id", "groups_malformed", "groups_repeated",
                "segments_placed", "segments_repeated", "segments_early_last", "objects_completed", "objects_mismatched",
                "objects_too_large", "slides_written", "slides_dropped", "xpad_bytes", "object_bytes")
MOT_RESULT_DTYPE = np.dtype([(n, np.int32) for n in MOT_COUNTERS] + [("reserved", np.int32, (8,))])
assert MOT_RESULT_DTYPE.itemsize == 128
MOT_CONTENT_IMAGE = 2
#: dabgpu_packet_result: what one entry of packet_slides_dev / packet_slides_host counted in one call; `mot` is a
#: MOT_RESULT_DTYPE record (from the closed data group on)
PACKET_COUNTERS = ("cifs", "slots", "slots_bad", "packets_fec", "packets_padding", "packets_other", "packets_followed",
                   "continuity_breaks", "packets_malformed", "packets_command", "packets_orphan", "groups_opened",
                   "groups_unfinished", "groups_too_long", "group_bytes")
PACKET_RESULT_DTYPE = np.dtype([(n, np.int32) for n in PACKET_COUNTERS] + [("reserved", np.int32), ("mot", MOT_RESULT_DTYPE)])
assert PACKET_RESULT_DTYPE.itemsize == 192
#: dabgpu_packet_carousel_result: what one entry of packet_carousel_dev / packet_carousel_host counted in one call; `head` is
#: a PACKET_RESULT_DTYPE record (the scan, the followed packets, the closed groups)
PACKET_CAROUSEL_COUNTERS = ("groups_header_mode", "groups_compressed_directory", "groups_unlisted", "directories_completed",
                            "directories_mismatched", "directories_too_large", "objects_stale", "objects_evicted", "objects_dropped",
                            "objects_deferred", "objects_written", "directory_id", "directory_bytes", "directory_objects",
                            "directory_period", "directory_segment_size")
PACKET_CAROUSEL_RESULT_DTYPE = np.dtype([("head", PACKET_RESULT_DTYPE)] + [(n, np.int32) for n in PACKET_CAROUSEL_COUNTERS])
assert PACKET_CAROUSEL_RESULT_DTYPE.itemsize == 256
#: dabgpu_mot_carousel_object: the record in front of every object in its slot (then header_bytes of MOT header, then the body)
MOT_CAROUSEL_OBJECT_DTYPE = np.dtype([(n, np.int32) for n in (
    "transport_id", "content_type", "content_subtype", "header_bytes", "body_bytes", "frame", "slot", "directory_id")])
assert MOT_CAROUSEL_OBJECT_DTYPE.itemsize == 32
#: dabgpu_mot_directory / dabgpu_mot_directory_object: what mot_directory_parse gives
MOT_DIRECTORY_DTYPE = np.dtype([(n, np.int32) for n in ("objects", "period", "segment_size", "extension_offset", "extension_bytes",
                                                        "directory_bytes")] + [("reserved", np.int32, (2,))])
MOT_DIRECTORY_OBJECT_DTYPE = np.dtype([(n, np.int32) for n in ("transport_id", "header_offset", "header_bytes", "body_bytes",
                                                               "content_type", "content_subtype")] + [("reserved", np.int32, (2,))])
assert MOT_DIRECTORY_DTYPE.itemsize == 32 and MOT_DIRECTORY_OBJECT_DTYPE.itemsize == 32
#: dabgpu_data_group: one emitted MSC data group of packet_groups_dev / packet_groups_host (mode 1: one continuity break)
DATA_GROUP_DTYPE = np.dtype([("offset", np.int32), ("length", np.int32), ("cif", np.int32), ("slot", np.uint8), ("type", np.uint8),
                             ("continuity", np.uint8), ("repetition", np.uint8), ("flags", np.uint16), ("extension", np.uint16),
                             ("segment", np.int32), ("transport_id", np.int32), ("data_offset", np.uint16), ("data_length", np.uint16)])
assert DATA_GROUP_DTYPE.itemsize == 32
DG_EXTENSION, DG_CRC, DG_SEGMENT, DG_USER_ACCESS, DG_TRANSPORT_ID, DG_REPEAT, DG_BREAK = 1, 2, 4, 8, 16, 32, 64
#: dabgpu_packet_groups_result: what one entry of packet_groups_dev / packet_groups_host counted in one call
PACKET_GROUPS_COUNTERS = PACKET_COUNTERS + ("groups_closed", "groups_malformed", "groups_crc_failed", "groups_no_crc", "groups_repeated",
                                            "groups_emitted", "groups_no_room", "bytes_emitted", "bytes_no_room")
PACKET_GROUPS_RESULT_DTYPE = np.dtype([(n, np.int32) for n in PACKET_GROUPS_COUNTERS] + [("reserved", np.int32, (4,))])
assert PACKET_GROUPS_RESULT_DTYPE.itemsize == 112
#: dabgpu_user_application: one (SId, SCIdS, user application type) of FIG 0/13, joined to its component
USER_APPLICATION_DTYPE = np.dtype([("sid", np.uint32), ("scids", np.int32), ("ua_type", np.int32), ("tmid_packet", np.int32),
                                   ("subchid", np.int32), ("scid", np.int32), ("packet_address", np.int32), ("data_length", np.int32),
                                   ("data", np.uint8, (23,)), ("reserved", np.uint8)])
assert USER_APPLICATION_DTYPE.itemsize == 56
#: registered user application types it is useful to know (TS 101 756); the library does not interpret them
UA_SLIDESHOW, UA_TPEG, UA_SPI, UA_FILECASTING, UA_JOURNALINE = 0x002, 0x004, 0x007, 0x00D, 0x44A
#: dabgpu_packet_component: one packet-mode service component (fig_packet_components)
PACKET_COMPONENT_DTYPE = np.dtype([("sid", np.uint32), ("scid", np.int32), ("subchid", np.int32), ("start_address", np.int32),
                                   ("packet_address", np.int32), ("dscty", np.int32), ("dg_flag", np.int32), ("fec_scheme", np.int32),
                                   ("primary", np.int32), ("reserved", np.int32, (3,))])
assert PACKET_COMPONENT_DTYPE.itemsize == 48
#: dabgpu_packet_fec_result: what one entry of packet_fec_dev / packet_fec_host counted in one call
PACKET_FEC_COUNTERS = ("cifs", "slots", "marks", "frames", "frames_cut", "frames_overlapping", "rows_clean", "rows_corrected",
                       "rows_uncorrectable", "bytes_corrected", "parity_bytes_corrected")
PACKET_FEC_RESULT_DTYPE = np.dtype([(n, np.int32) for n in PACKET_FEC_COUNTERS] + [("reserved", np.int32)])
assert PACKET_FEC_RESULT_DTYPE.itemsize == 48
#: dabgpu_packet_fec_erasure_result: the twelve words above, then what packet_fec_erasures_dev / _host add
PACKET_FEC_ERASURE_COUNTERS = PACKET_FEC_COUNTERS + ("slots_suspect", "frames_with_suspects", "frames_beyond_erasures", "rows_erasure_corrected",
                                                     "erased_bytes_changed", "erasure_other_bytes_corrected")
PACKET_FEC_ERASURE_RESULT_DTYPE = np.dtype([(n, np.int32) for n in PACKET_FEC_COUNTERS] + [("reserved", np.int32)] +
                                           [(n, np.int32) for n in PACKET_FEC_ERASURE_COUNTERS[len(PACKET_FEC_COUNTERS):]] + [("reserved2", np.int32, (2,))])
assert PACKET_FEC_ERASURE_RESULT_DTYPE.itemsize == 80
DSCTY_MOT = 60
#: dabgpu_audio_component: one MSC stream audio component (fig_audio_components)
AUDIO_COMPONENT_DTYPE = np.dtype([("sid", np.uint32), ("subchid", np.int32), ("start_address", np.int32), ("ascty", np.int32),
                                  ("primary", np.int32), ("reserved", np.int32, (3,))])
assert AUDIO_COMPONENT_DTYPE.itemsize == 32
ASCTY_DAB, ASCTY_DABPLUS = 0, 63
#: dabgpu_tii_acc: a stream's transmitter-identification sums (device memory; zero it to start), or one frame's record
TII_ACC_DTYPE = np.dtype([("cell", np.float32, (24, 8)), ("floor", np.float32), ("frames", np.int32), ("reserved", np.int32, (2,))])
assert TII_ACC_DTYPE.itemsize == 784
#: dabgpu_tii_entry: one transmitter found by tii_decode
TII_ENTRY_DTYPE = np.dtype([("main_id", np.int32), ("sub_id", np.int32), ("level_db", np.float32), ("flags", np.int32)])
assert TII_ENTRY_DTYPE.itemsize == 16
TII_AMBIGUOUS = 1
#: dabgpu_cir_acc: a stream's channel-impulse-response sums (device memory; zero it to start), or one frame's record
CIR_ACC_DTYPE = np.dtype([("tap", np.float32, (2048,)), ("carrier", np.float32, (1536,)), ("frames", np.int32),
                          ("reserved", np.int32, (3,))])
assert CIR_ACC_DTYPE.itemsize == 14352
#: dabgpu_cir_report: what cir_analyse found in one accumulator
CIR_REPORT_DTYPE = np.dtype([("frames", np.int32), ("n_paths", np.int32), ("floor", np.float32), ("peak", np.float32),
                             ("first_delay", np.float32), ("strongest_delay", np.float32), ("rms_delay_spread", np.float32),
                             ("guard_ratio_db", np.float32)])
assert CIR_REPORT_DTYPE.itemsize == 32
#: dabgpu_cir_path: one path found by cir_analyse
CIR_PATH_DTYPE = np.dtype([("delay", np.float32), ("level_db", np.float32), ("snr_db", np.float32), ("flags", np.int32)])
assert CIR_PATH_DTYPE.itemsize == 16
CIR_BEYOND_GUARD = 1
#: ETI(NI) output (include/dabgpu.h, "ETI(NI) output"): one 6144-byte frame per CIF
ETI_FRAME_BYTES = 6144
ETI_MAX_STREAMS = 64
ETI_FIC_DELAY = 15
ETI_WARMUP, ETI_FIB_CRC, ETI_NO_ANCHOR, ETI_COUNT_MISMATCH = 1, 2, 4, 8
#: dabgpu_eti_status: one frame's record
ETI_STATUS_DTYPE = np.dtype([("cif_count", np.uint16), ("flags", np.uint8), ("fib_ok", np.uint8), ("length", np.uint16),
                             ("reserved", np.uint16)])
assert ETI_STATUS_DTYPE.itemsize == 8
#: dabgpu_eti_history: a stream's FIC delay line between two calls (device memory; all zero = a stream that starts)
ETI_HISTORY_DTYPE = np.dtype([("fib", np.uint8, (15, 96)), ("crc_ok", np.uint8, (15, 3)), ("pad", np.uint8, (3,)),
                              ("next_count", np.int32), ("valid", np.int32), ("reserved", np.int32, (2,))])
assert ETI_HISTORY_DTYPE.itemsize == 1504
ETI_PARSE_ERRORS = {1: "FSYNC wrong, or not the pattern FCT's parity asks for", 2: "FICF / MID / NST / FL inconsistent",
                    3: "header CRC", 4: "data CRC"}
#: Mode I sample rate, samples per microsecond
SAMPLES_PER_US = 2.048


def mer_db(rec):
    """MER in dB of MER_DTYPE record(s): 10 log10(signal / error); +inf where error == 0, nan where no carrier counted."""
    rec = np.asarray(rec)
    sig = rec["signal"].astype(np.float64)
    err = rec["error"].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        db = 10.0 * np.log10(sig / err)
    return np.where(rec["carriers"] > 0, db, np.nan)


def ber(counts):
    """Bit-error rate of BER_DTYPE counts, summed over all of them (nan when no bit was counted)."""
    counts = np.asarray(counts)
    bits = int(counts["bits"].sum(dtype=np.uint64))
    return float(counts["errors"].sum(dtype=np.uint64)) / bits if bits else float("nan")


class DabplusEntry(C.Structure):
    """dabgpu_dabplus_entry: one followed DAB+ sub-channel of Context.dabplus_follow_dev (device addresses)."""
    _fields_ = [("d_in", C.c_void_p), ("in_stride", C.c_size_t), ("bitrate_kbps", C.c_int32), ("d_carry_in", C.c_void_p),
                ("d_carry_out", C.c_void_p), ("d_data", C.c_void_p), ("d_status", C.c_void_p), ("d_result", C.c_void_p)]


class Mp2Entry(C.Structure):
    """dabgpu_mp2_entry: one followed DAB (MPEG layer II) sub-channel of Context.mp2_follow_dev (device addresses) or
    mp2_follow_host (host addresses)."""
    _fields_ = [("d_in", C.c_void_p), ("in_stride", C.c_size_t), ("bitrate_kbps", C.c_int32), ("d_carry_in", C.c_void_p),
                ("d_carry_out", C.c_void_p), ("d_rows", C.c_void_p), ("d_status", C.c_void_p), ("d_follow", C.c_void_p),
                ("d_result", C.c_void_p)]


class Mp2AudioEntry(C.Structure):
    """dabgpu_mp2_audio_entry: one followed DAB (MPEG layer II) sub-channel of Context.mp2_subbands_dev (device addresses) or
    mp2_subbands_host (host addresses): the follow entry's d_in / d_carry_in / d_status / d_result, the level records, the
    optional sub-band samples, the counters."""
    _fields_ = [("d_in", C.c_void_p), ("in_stride", C.c_size_t), ("bitrate_kbps", C.c_int32), ("d_carry_in", C.c_void_p),
                ("d_status", C.c_void_p), ("d_result", C.c_void_p), ("d_levels", C.c_void_p), ("d_subbands", C.c_void_p),
                ("d_audio", C.c_void_p)]


class PadEntry(C.Structure):
    """dabgpu_pad_entry: one followed DAB+ sub-channel of Context.pad_labels_dev (device addresses) or pad_labels_host
    (host addresses): the follow entry's d_data / d_status / d_result, the state records, the label and the counters."""
    _fields_ = [("d_data", C.c_void_p), ("data_stride", C.c_size_t), ("d_status", C.c_void_p), ("d_follow", C.c_void_p),
                ("bitrate_kbps", C.c_int32), ("max_superframes", C.c_int32), ("d_state_in", C.c_void_p),
                ("d_state_out", C.c_void_p), ("d_label", C.c_void_p), ("d_result", C.c_void_p)]


class MotEntry(C.Structure):
    """dabgpu_mot_entry: one followed DAB+ sub-channel of Context.mot_slides_dev (device addresses) or mot_slides_host (host
    addresses): the follow entry's d_data / d_status / d_result, the state records, the arena, the slide slots, the counters."""
    _fields_ = [("d_data", C.c_void_p), ("data_stride", C.c_size_t), ("d_status", C.c_void_p), ("d_follow", C.c_void_p),
                ("bitrate_kbps", C.c_int32), ("max_superframes", C.c_int32), ("d_state_in", C.c_void_p),
                ("d_state_out", C.c_void_p), ("d_arena", C.c_void_p), ("arena_bytes", C.c_size_t), ("d_slides", C.c_void_p),
                ("slide_stride", C.c_size_t), ("max_slides", C.c_int32), ("reserved", C.c_int32), ("d_result", C.c_void_p)]


class PacketEntry(C.Structure):
    """dabgpu_packet_entry: one (sub-channel, packet address) of Context.packet_slides_dev (device addresses) or
    packet_slides_host (host addresses): the logical frames the decode call wrote, the address followed, the state records,
    the arena, the slide slots, the counters."""
    _fields_ = [("d_in", C.c_void_p), ("in_stride", C.c_size_t), ("bitrate_kbps", C.c_int32), ("address", C.c_int32),
                ("fec", C.c_int32), ("reserved", C.c_int32), ("d_state_in", C.c_void_p), ("d_state_out", C.c_void_p),
                ("d_arena", C.c_void_p), ("arena_bytes", C.c_size_t), ("d_slides", C.c_void_p), ("slide_stride", C.c_size_t),
                ("max_slides", C.c_int32), ("reserved2", C.c_int32), ("d_result", C.c_void_p)]


class PacketCarouselEntry(C.Structure):
    """dabgpu_packet_carousel_entry: one (sub-channel, packet address) of Context.packet_carousel_dev (device addresses) or
    packet_carousel_host (host addresses): the fields of PacketEntry, the three sizes (directory_capacity, assemblies,
    object_capacity), the object slots and the directory buffer."""
    _fields_ = [("d_in", C.c_void_p), ("in_stride", C.c_size_t), ("bitrate_kbps", C.c_int32), ("address", C.c_int32),
                ("fec", C.c_int32), ("assemblies", C.c_int32), ("d_state_in", C.c_void_p), ("d_state_out", C.c_void_p),
                ("d_arena", C.c_void_p), ("arena_bytes", C.c_size_t), ("d_objects", C.c_void_p), ("object_stride", C.c_size_t),
                ("max_objects", C.c_int32), ("object_capacity", C.c_int32), ("d_directory", C.c_void_p),
                ("directory_capacity", C.c_int32), ("reserved", C.c_int32), ("d_result", C.c_void_p)]


class PacketGroupsEntry(C.Structure):
    """dabgpu_packet_groups_entry: one (sub-channel, packet address) of Context.packet_groups_dev (device addresses) or
    packet_groups_host (host addresses): the logical frames, the address followed, mode (0 data groups, 1 raw bytes),
    keep_repeats, the state records, the bytes and records that come out, the counters."""
    _fields_ = [("d_in", C.c_void_p), ("in_stride", C.c_size_t), ("bitrate_kbps", C.c_int32), ("address", C.c_int32),
                ("fec", C.c_int32), ("mode", C.c_int32), ("keep_repeats", C.c_int32), ("reserved", C.c_int32),
                ("d_state_in", C.c_void_p), ("d_state_out", C.c_void_p), ("d_bytes", C.c_void_p), ("d_groups", C.c_void_p),
                ("bytes_capacity", C.c_int32), ("max_groups", C.c_int32), ("d_result", C.c_void_p)]


class PacketFecEntry(C.Structure):
    """dabgpu_packet_fec_entry: one FEC-protected packet sub-channel of Context.packet_fec_dev (device addresses) or
    packet_fec_host (host addresses): the logical frames the decode call wrote, the corrected frames (delayed by
    packet_fec_delay(bitrate) frames; what the slides call then names as d_in), the state records, the counters."""
    _fields_ = [("d_in", C.c_void_p), ("in_stride", C.c_size_t), ("bitrate_kbps", C.c_int32), ("reserved", C.c_int32),
                ("d_out", C.c_void_p), ("out_stride", C.c_size_t), ("d_state_in", C.c_void_p), ("d_state_out", C.c_void_p),
                ("d_result", C.c_void_p)]


class PacketFecErasureEntry(C.Structure):
    """dabgpu_packet_fec_erasure_entry: the fields of PacketFecEntry for Context.packet_fec_erasures_dev (device addresses) or
    packet_fec_erasures_host (host addresses); d_result is a PACKET_FEC_ERASURE_RESULT_DTYPE record.  The state record has
    the size packet_fec_state_bytes(bitrate) gives; one written by the errors-only call is a fresh start here."""
    _fields_ = list(PacketFecEntry._fields_)


class StreamComponent(C.Structure):
    """dabgpu_stream_component: a stream-mode data component (FIG 0/2 TMId 1) joined to FIG 0/1"""
    _fields_ = [("sid", C.c_uint32), ("subchid", C.c_int32), ("start_address", C.c_int32), ("dscty", C.c_int32),
                ("primary", C.c_int32), ("ca", C.c_int32), ("reserved", C.c_int32 * 2)]


TS_MAX_PROGRAMS, TS_MAX_STREAMS = 16, 16


class TsProgram(C.Structure):
    """dabgpu_ts_program: a programme of the PAT and, when pmt_seen, of its PMT"""
    _fields_ = [("program_number", C.c_int32), ("pmt_pid", C.c_int32), ("pmt_seen", C.c_int32), ("pcr_pid", C.c_int32),
                ("iod_present", C.c_int32), ("n_streams", C.c_int32), ("stream_type", C.c_int32 * TS_MAX_STREAMS),
                ("stream_pid", C.c_int32 * TS_MAX_STREAMS)]


class TsInfo(C.Structure):
    """dabgpu_ts_info: what dabgpu_ts_programs found in a buffer of TS packets"""
    _fields_ = [("transport_stream_id", C.c_int32), ("network_pid", C.c_int32), ("n_programs", C.c_int32),
                ("pat_sections", C.c_int32), ("pmt_sections", C.c_int32), ("crc_errors", C.c_int32), ("reserved", C.c_int32 * 2),
                ("programs", TsProgram * TS_MAX_PROGRAMS)]


class DmbEntry(C.Structure):
    """dabgpu_dmb_entry: one T-DMB stream-mode sub-channel of Context.dmb_follow_dev (device addresses) or dmb_follow_host
    (host addresses): the logical frames, room for max_packets TS packets of 188 bytes and as many DMB_RECORD_DTYPE records
    (dmb_max_packets(bitrate, n_cifs) holds everything; with less, up to DMB_DEFER_ROOM packets wait in the state record), the state records (dmb_state_bytes()), a DMB_RESULT_DTYPE record."""
    _fields_ = [("d_in", C.c_void_p), ("in_stride", C.c_size_t), ("bitrate_kbps", C.c_int32), ("max_packets", C.c_int32),
                ("d_ts", C.c_void_p), ("d_records", C.c_void_p), ("d_state_in", C.c_void_p), ("d_state_out", C.c_void_p),
                ("d_result", C.c_void_p)]


class PacketComponent(C.Structure):
    _fields_ = [("sid", C.c_uint32), ("scid", C.c_int32), ("subchid", C.c_int32), ("start_address", C.c_int32),
                ("packet_address", C.c_int32), ("dscty", C.c_int32), ("dg_flag", C.c_int32), ("fec_scheme", C.c_int32),
                ("primary", C.c_int32), ("reserved", C.c_int32 * 3)]


assert C.sizeof(PacketComponent) == PACKET_COMPONENT_DTYPE.itemsize


class MotText(C.Structure):
    _fields_ = [("length", C.c_int32), ("bytes", C.c_uint8 * 256)]


class MotHeader(C.Structure):
    """dabgpu_mot_header: what mot_header_parse reads from the MOT header of a slide"""
    _fields_ = [("body_size", C.c_int32), ("header_size", C.c_int32), ("content_type", C.c_int32), ("content_subtype", C.c_int32),
                ("n_params", C.c_int32), ("n_unknown", C.c_int32), ("name_charset", C.c_int32), ("has_trigger", C.c_int32),
                ("trigger_now", C.c_int32), ("trigger_time", C.c_uint32), ("has_expire", C.c_int32), ("expire_now", C.c_int32),
                ("expire_time", C.c_uint32), ("has_category", C.c_int32), ("category_id", C.c_int32), ("slide_id", C.c_int32),
                ("name", MotText), ("category_title", MotText), ("click_through_url", MotText), ("alternative_location_url", MotText)]


class AudioComponent(C.Structure):
    _fields_ = [("sid", C.c_uint32), ("subchid", C.c_int32), ("start_address", C.c_int32), ("ascty", C.c_int32),
                ("primary", C.c_int32), ("reserved", C.c_int32 * 3)]


assert C.sizeof(AudioComponent) == AUDIO_COMPONENT_DTYPE.itemsize


class SyncResult(C.Structure):
    _fields_ = [("coarse_carriers", C.c_int32), ("time_offset", C.c_int32), ("peak_to_mean", C.c_float),
                ("coarse_peak_to_mean", C.c_float)]


class AcquireCfg(C.Structure):
    _fields_ = [("thr_null_start", C.c_float), ("thr_null_end", C.c_float), ("min_null_blocks", C.c_int32),
                ("max_coarse_carriers", C.c_int32), ("min_peak_to_mean", C.c_float), ("timing_margin", C.c_int32),
                ("impulse_peak_distance_probability", C.c_float), ("first_path_rel", C.c_float),
                ("level_chunk_blocks", C.c_int32), ("reserved", C.c_int32)]


class TrackCfg(C.Structure):
    _fields_ = [("fine_freq_update_beta", C.c_float), ("signal_update_beta", C.c_float), ("thr_null_start", C.c_float),
                ("min_peak_to_mean", C.c_float), ("impulse_peak_distance_probability", C.c_float),
                ("first_path_rel", C.c_float), ("drift_beta", C.c_float), ("coarse_freq_slow_beta", C.c_float),
                ("timing_margin", C.c_int32), ("max_coarse_carriers", C.c_int32), ("decision_directed", C.c_int32), ("auto_acquire", C.c_int32),
                ("dd_gate", C.c_float), ("reserved", C.c_int32)]


class PlacementReport(C.Structure):
    _fields_ = [("method", C.c_int32), ("fallback_reason", C.c_int32), ("n_chunks", C.c_int32), ("iq_chunks", C.c_int32),
                ("soft_chunks", C.c_int32), ("n_domains", C.c_int32), ("conflicts", C.c_int32), ("runtime_error", C.c_int32),
                ("chunk_bytes", C.c_uint64), ("setup_peak_bytes", C.c_uint64),
                ("classify_ms", C.c_float), ("pair_over_same_domain", C.c_float),
                ("domains", C.c_char * 100), ("iq_map", C.c_char * 72), ("soft_map", C.c_char * 28)]


class FrameResult(C.Structure):
    _fields_ = [("sync", SyncResult), ("flags", C.c_int32), ("reserved", C.c_int32), ("stats", Stats)]


ACQUIRED_FRAME_DTYPE = np.dtype([("start", np.int64), ("freq_offset", np.float32), ("coarse_carriers", np.int32),
                                 ("fine_offset", np.float32), ("peak_to_mean", np.float32),
                                 ("coarse_peak_to_mean", np.float32), ("flags", np.int32)])     # 32 bytes


class TiiCfg(C.Structure):
    _fields_ = [("min_level_db", C.c_float), ("reserved", C.c_int32)]


def tii_pattern(p):
    """8-bit mask of TII pattern p (main identifier 0..69; bit 7 - b = position b), -1 outside the table: the library's own."""
    return int(lib().dabgpu_tii_pattern(int(p)))


def tii_decode(acc, min_level_db=3.0, max_out=24 * 70):
    """Transmitters in one TII_ACC_DTYPE accumulator (a host copy) -> TII_ENTRY_DTYPE array, strongest first
    (dabgpu_tii_decode: host only, no GPU)."""
    acc = np.ascontiguousarray(np.asarray(acc, TII_ACC_DTYPE).reshape(()))
    cfg = TiiCfg()
    lib().dabgpu_tii_default_cfg(C.byref(cfg))
    cfg.min_level_db = min_level_db
    out = np.zeros(max_out, TII_ENTRY_DTYPE)
    n = lib().dabgpu_tii_decode(_p(acc), C.byref(cfg), _p(out), max_out)
    if n < 0:
        raise DabGpuError(n, "dabgpu_tii_decode")
    return out[:min(n, max_out)].copy()


class CirCfg(C.Structure):
    _fields_ = [("min_snr_db", C.c_float), ("range_db", C.c_float)]


def cir_analyse(acc, min_snr_db=10.0, range_db=25.0, max_out=64):
    """Paths in one CIR_ACC_DTYPE accumulator (a host copy) -> (report CIR_REPORT_DTYPE, paths CIR_PATH_DTYPE array by
    delay ascending) (dabgpu_cir_analyse: host only, no GPU)."""
    acc = np.ascontiguousarray(np.asarray(acc, CIR_ACC_DTYPE).reshape(()))
    cfg = CirCfg(min_snr_db, range_db)
    report = np.zeros((), CIR_REPORT_DTYPE)
    out = np.zeros(max(max_out, 1), CIR_PATH_DTYPE)
    n = lib().dabgpu_cir_analyse(_p(acc), C.byref(cfg), _p(report), _p(out), max_out)
    if n < 0:
        raise DabGpuError(n, "dabgpu_cir_analyse")
    return report[()], out[:min(n, max_out)].copy()


def samples_to_us(samples):
    """Delay in samples (2.048 MHz, Mode I) -> microseconds."""
    return np.asarray(samples, np.float64) / SAMPLES_PER_US


def samples_to_km(samples):
    """Delay in samples -> the extra path length it stands for, km (light travels 0.299792458 km per microsecond)."""
    return samples_to_us(samples) * 0.299792458


def soft_selection(subchannels, with_fic=True):
    """[(first_bit, count), ...] covering the FIC and the given sub-channels (dabgpu_soft_selection)."""
    n = len(subchannels)
    arr = (Subchannel * max(n, 1))(*subchannels)
    out = np.zeros((1 + 4 * n, 2), np.int32)
    k = lib().dabgpu_soft_selection(arr, n, int(bool(with_fic)), _p(out), len(out))
    _check(min(k, 0), "dabgpu_soft_selection")
    return [tuple(int(v) for v in r) for r in out[:k]]


def acquire_cfg(**kw):
    """dabgpu_acquire_default_cfg(), then the given fields overridden."""
    c = AcquireCfg()
    lib().dabgpu_acquire_default_cfg(C.byref(c))
    for k, v in kw.items():
        if not hasattr(c, k):
            raise AttributeError(k)
        setattr(c, k, v)
    return c


def track_cfg(**kw):
    """dabgpu_track_default_cfg(), then the given fields overridden."""
    c = TrackCfg()
    lib().dabgpu_track_default_cfg(C.byref(c))
    for k, v in kw.items():
        if not hasattr(c, k):
            raise AttributeError(k)
        setattr(c, k, v)
    return c


class Subchannel(C.Structure):
    _fields_ = [("start_address", C.c_int32), ("length", C.c_int32), ("is_uep", C.c_int32),
                ("eep_type", C.c_int32), ("protection_level", C.c_int32), ("bitrate_kbps", C.c_int32)]


class EtiStream(C.Structure):
    """One stream of an ETI frame: the sub-channel's id (FIG 0/1) and its descriptor."""
    _fields_ = [("subchannel_id", C.c_int32), ("sc", Subchannel)]


class EtiPlan(C.Structure):
    _fields_ = [("nst", C.c_int32), ("fl", C.c_int32), ("header_bytes", C.c_int32), ("data_bytes", C.c_int32),
                ("length", C.c_int32), ("reserved", C.c_int32 * 3), ("order", C.c_int32 * 64), ("offset", C.c_int32 * 64),
                ("bytes", C.c_int32 * 64), ("header", C.c_uint8 * 272)]


class EtiInfo(C.Structure):
    _fields_ = [("err", C.c_int32), ("fct", C.c_int32), ("fp", C.c_int32), ("mid", C.c_int32), ("nst", C.c_int32),
                ("fl", C.c_int32), ("length", C.c_int32), ("fic_offset", C.c_int32), ("header_crc", C.c_int32),
                ("data_crc", C.c_int32), ("reserved", C.c_int32 * 2), ("scid", C.c_int32 * 64), ("sad", C.c_int32 * 64),
                ("tpl", C.c_int32 * 64), ("stl", C.c_int32 * 64), ("offset", C.c_int32 * 64)]


def eti_layout(streams):
    """Validate sub-channels [(subchannel_id, Subchannel) or EtiStream, ...] for an ETI frame and lay the frame out
    (dabgpu_eti_layout: host only, no GPU) -> EtiPlan; plan.order[k] is the index in `streams` of the frame's k-th
    stream (ascending start address).  DabGpuError (ERR_ARG) for a configuration an ETI frame cannot carry."""
    items = [s if isinstance(s, EtiStream) else EtiStream(int(s[0]), s[1]) for s in streams]
    arr = (EtiStream * max(len(items), 1))(*items)
    plan = EtiPlan()
    _check(lib().dabgpu_eti_layout(arr, len(items), C.byref(plan)), "dabgpu_eti_layout")
    return plan


def eti_history_bytes():
    return int(lib().dabgpu_eti_history_bytes())


#: ETI(NI) input (include/dabgpu.h, "ETI(NI) input"): verdicts of a row beside 0 (taken), flags of its status
ETI_BAD_DATA_CRC, ETI_OTHER_PLAN = 4, 5
ETI_READ_GAP, ETI_READ_FP_BREAK, ETI_READ_ERR_FIELD, ETI_READ_FIB_CRC = 1, 2, 4, 8
#: dabgpu_eti_read_status: one emitted row
ETI_READ_STATUS_DTYPE = np.dtype([("offset", np.uint32), ("verdict", np.uint8), ("fct", np.uint8), ("fp", np.uint8), ("err", np.uint8),
                                  ("fib_ok", np.uint8), ("gap", np.uint8), ("flags", np.uint8), ("reserved", np.uint8),
                                  ("reserved2", np.uint32)])
assert ETI_READ_STATUS_DTYPE.itemsize == 16
#: dabgpu_eti_read_result: what one entry of eti_read_dev / eti_read_host counted in one call
ETI_READ_RESULT_DTYPE = np.dtype([(f, np.uint32) for f in ("rows", "taken", "bad_data_crc", "other_plan", "skipped", "resyncs",
                                                           "gap_sum", "fib_errors", "tail_bytes")] + [("reserved", np.uint32, (3,))])
assert ETI_READ_RESULT_DTYPE.itemsize == 48
#: the head of a state record of eti_read_dev / eti_read_host; the tail's bytes follow it
ETI_READ_HEAD_DTYPE = np.dtype([("tail_bytes", np.uint32), ("have_prev", np.uint8), ("last_fct", np.uint8), ("last_fp", np.uint8),
                                ("reserved", np.uint8)] + [(f, np.uint64) for f in ("rows", "taken", "bad_data_crc", "other_plan",
                                                                                    "skipped", "resyncs", "gap_sum", "fib_errors",
                                                                                    "reserved2")])
assert ETI_READ_HEAD_DTYPE.itemsize == 80


class EtiReadEntry(C.Structure):
    """dabgpu_eti_read_entry: one byte stream of Context.eti_read_dev (device addresses) or eti_read_host (host addresses).
    plan: C.pointer(EtiPlan) or None (discovery: only the FIC leaves); d_out: an array of plan.nst addresses (C.c_void_p *
    nst) in the order the streams were given to eti_layout, 0 = not wanted, or None.  The Python objects behind plan and
    d_out must stay alive until the call has returned."""
    _fields_ = [("d_bytes", C.c_void_p), ("n_bytes", C.c_int32), ("reserved", C.c_int32), ("plan", C.POINTER(EtiPlan)),
                ("d_out", C.POINTER(C.c_void_p)), ("d_state_in", C.c_void_p), ("d_state_out", C.c_void_p), ("d_fib", C.c_void_p),
                ("d_crc_ok", C.c_void_p), ("d_status", C.c_void_p), ("d_result", C.c_void_p)]


def eti_read_state_bytes():
    """Bytes of one state record of Context.eti_read_dev / eti_read_host (all zero = a stream that starts)."""
    return int(lib().dabgpu_eti_read_state_bytes())


def eti_read_max_frames(n_bytes):
    """Rows one entry can emit in one call: its outputs hold this many."""
    return (6143 + int(n_bytes)) // ETI_FRAME_BYTES


def eti_read_host(entries):
    """Context.eti_read_dev on HOST memory (entries: EtiReadEntry with host addresses): the same checks and the same walk,
    serially, without a context or a GPU (dabgpu_eti_read_host)."""
    _entries_call("dabgpu_eti_read_host", EtiReadEntry, entries)


#: EDI (include/dabgpu.h, "EDI output" / "EDI input"; include/dabgpu_edi.h): AF packets, one per CIF
EDI_MAX_PACKET = 8192
EDI_BAD_HEADER, EDI_BAD_CRC, EDI_BAD_TAGS, EDI_NOT_DETI = 1, 2, 3, 4
EDI_PARSE_ERRORS = {1: "not an AF packet of this length (SYNC, LEN, AR, PT)", 2: "CRC", 3: "malformed TAG items",
                    4: "not a DETI packet"}
EDI_READ_GAP, EDI_READ_SEQ_BREAK, EDI_READ_FP_MISMATCH, EDI_READ_STAT_FIELD = 1, 2, 4, 8
EDI_READ_FIB_CRC, EDI_READ_NO_FIC, EDI_READ_TIME = 16, 32, 64
#: dabgpu_edi_read_status: one emitted row
EDI_READ_STATUS_DTYPE = np.dtype([("offset", np.uint32), ("length", np.uint16), ("dlfc", np.uint16), ("seq", np.uint16),
                                  ("gap", np.uint16), ("fp", np.uint8), ("stat", np.uint8), ("mid", np.uint8), ("fib_ok", np.uint8),
                                  ("flags", np.uint8), ("utco", np.uint8), ("reserved", np.uint8, (2,)), ("seconds", np.uint32),
                                  ("tsta", np.uint32), ("reserved2", np.uint32)])
assert EDI_READ_STATUS_DTYPE.itemsize == 32
#: dabgpu_edi_read_result: what one entry of edi_read_host counted in one call
EDI_READ_RESULT_DTYPE = np.dtype([(f, np.uint32) for f in ("rows", "not_deti", "bad_tags", "other_plan", "skipped", "resyncs",
                                                           "gap_sum", "fib_errors", "tail_bytes")] + [("reserved", np.uint32, (3,))])
assert EDI_READ_RESULT_DTYPE.itemsize == 48
#: the head of a state record of edi_read_host; the tail's 8192 bytes follow it
EDI_READ_HEAD_DTYPE = np.dtype([("tail_bytes", np.uint32), ("have_prev", np.uint8), ("have_seq", np.uint8), ("in_skip", np.uint8),
                                ("reserved", np.uint8), ("last_dlfc", np.uint16), ("last_seq", np.uint16), ("reserved1", np.uint32)] +
                               [(f, np.uint64) for f in ("rows", "not_deti", "bad_tags", "other_plan", "skipped", "resyncs", "gap_sum",
                                                         "fib_errors")] + [("reserved2", np.uint64, (2,))])
assert EDI_READ_HEAD_DTYPE.itemsize == 96


class EdiInfo(C.Structure):
    _fields_ = [(f, C.c_int32) for f in ("len", "length", "seq", "crc", "n_ptr", "n_deti", "n_other", "atstf", "ficf", "rfudf", "dlfc",
                                         "stat", "mid", "fp", "mnsc", "utco", "tsta")] + \
               [("seconds", C.c_uint32), ("fic_offset", C.c_int32), ("nst", C.c_int32), ("reserved", C.c_int32 * 4),
                ("scid", C.c_int32 * 64), ("sad", C.c_int32 * 64), ("tpl", C.c_int32 * 64), ("stl", C.c_int32 * 64),
                ("offset", C.c_int32 * 64)]


class EdiReadEntry(EtiReadEntry):
    """dabgpu_edi_read_entry: one byte stream of edi_read_host (host addresses); the fields of EtiReadEntry, d_fib / d_crc_ok /
    d_status sized by edi_read_max_rows.  The Python objects behind plan and d_out must stay alive until the call has
    returned."""


def _edi_bytes(packet):
    return np.ascontiguousarray(np.frombuffer(bytes(packet), np.uint8) if isinstance(packet, (bytes, bytearray)) else packet,
                                np.uint8).reshape(-1)


def edi_packet_bytes(plan):
    """Bytes of the one AF packet size a plan's CIFs are written as (dabgpu_edi_packet_bytes: host only)."""
    n = lib().dabgpu_edi_packet_bytes(C.byref(plan))
    _check(min(n, 0), "dabgpu_edi_packet_bytes")
    return n


def edi_parse(packet):
    """Check one AF packet (header, CRC, TAG items, what makes it a DETI packet; dabgpu_edi_parse: host only) and give its
    parts: dict with len, length, seq, crc, dlfc, stat, mid, fp, mnsc, atstf, ficf, rfudf, utco, seconds, tsta, nst, streams
    [{scid, sad, tpl, stl, data}], fic (96 bytes or None).  ValueError for anything else; its args[1] is the DABGPU_EDI_* code."""
    f = _edi_bytes(packet)
    info = EdiInfo()
    rc = lib().dabgpu_edi_parse(_p(f), f.size, C.byref(info))
    if rc < 0:
        raise DabGpuError(rc, "dabgpu_edi_parse")
    if rc > 0:
        raise ValueError("not a DETI packet: " + EDI_PARSE_ERRORS.get(rc, str(rc)), rc)
    streams = [{"scid": info.scid[k], "sad": info.sad[k], "tpl": info.tpl[k], "stl": info.stl[k],
                "data": f[info.offset[k]:info.offset[k] + 8 * info.stl[k]].copy()} for k in range(info.nst)]
    out = {k: getattr(info, k) for k in ("len", "length", "seq", "crc", "n_ptr", "n_deti", "n_other", "atstf", "ficf", "rfudf", "dlfc",
                                         "stat", "mid", "fp", "mnsc", "utco", "tsta", "seconds", "nst")}
    out["fic"] = f[info.fic_offset:info.fic_offset + 96].copy() if info.fic_offset >= 0 else None
    out["streams"] = streams
    return out


def edi_streams(packet):
    """The stream list of one DETI packet, read back from its est items (dabgpu_edi_streams_from_packet: host only):
    [EtiStream, ...] in the packet's order, what eti_layout takes."""
    f = _edi_bytes(packet)
    arr = (EtiStream * ETI_MAX_STREAMS)()
    n = C.c_int(0)
    _check(lib().dabgpu_edi_streams_from_packet(_p(f), f.size, arr, C.byref(n)), "dabgpu_edi_streams_from_packet")
    return [EtiStream(arr[k].subchannel_id, arr[k].sc) for k in range(n.value)]


def edi_read_state_bytes():
    """Bytes of one state record of edi_read_host (all zero = a stream that starts)."""
    return int(lib().dabgpu_edi_read_state_bytes())


def edi_read_max_rows(n_bytes, plan=None):
    """Rows one entry of edi_read_host can emit in one call: its outputs hold this many (plan None: discovery)."""
    n = lib().dabgpu_edi_read_max_rows(int(n_bytes), None if plan is None else C.byref(plan))
    _check(min(n, 0), "dabgpu_edi_read_max_rows")
    return n


def edi_read_host(entries):
    """AF packet byte streams -> FIBs, CRC flags and logical frames on HOST memory (entries: EdiReadEntry with host
    addresses), serially, without a context or a GPU (dabgpu_edi_read_host)."""
    _entries_call("dabgpu_edi_read_host", EtiReadEntry, entries)


#: EDI PFT layer (include/dabgpu.h, "EDI PFT layer"; include/dabgpu_pft.h): PF fragments with RS(255,207), EDI over UDP
PFT_FEC, PFT_ADDR, PFT_RECOVERED, PFT_INCONSISTENT, PFT_LOST, PFT_AF_OK, PFT_FLUSHED = 1, 2, 4, 8, 16, 32, 64
PFT_READ_FLUSH = 1
#: dabgpu_pft_read_record: one closed group that held a fragment
PFT_READ_RECORD_DTYPE = np.dtype([("offset", np.uint32), ("length", np.uint16), ("pseq", np.uint16), ("fcount", np.uint16),
                                  ("received", np.uint16), ("plen", np.uint16), ("rs_k", np.uint8), ("rs_z", np.uint8),
                                  ("chunks", np.uint8), ("max_erasures", np.uint8), ("flags", np.uint16), ("source", np.uint16),
                                  ("dest", np.uint16), ("reserved", np.uint32, (2,))])
assert PFT_READ_RECORD_DTYPE.itemsize == 32
#: dabgpu_pft_read_result: what one entry of pft_read_dev / pft_read_host counted in one call
PFT_READ_RESULT_DTYPE = np.dtype([(f, np.uint32) for f in ("records", "packets", "lost", "recovered", "fragments", "duplicates",
                                                           "mismatched", "late", "unsupported", "missing", "skipped", "resyncs",
                                                           "out_bytes", "tail_bytes", "chunks_filled", "bytes_filled")])
assert PFT_READ_RESULT_DTYPE.itemsize == 64
#: the head of a state record of pft_read_dev / pft_read_host; the two open groups and the tail follow it
PFT_READ_HEAD_DTYPE = np.dtype([("tail_bytes", np.uint32), ("have_horizon", np.uint8), ("in_skip", np.uint8), ("late_run", np.uint8),
                                ("reserved", np.uint8), ("horizon", np.uint16), ("reserved1", np.uint16), ("reserved2", np.uint32)] +
                               [(f, np.uint64) for f in ("records", "packets", "lost", "recovered", "fragments", "duplicates",
                                                         "mismatched", "late", "unsupported", "missing", "skipped", "resyncs",
                                                         "out_bytes", "chunks_filled", "bytes_filled", "reserved3")])
assert PFT_READ_HEAD_DTYPE.itemsize == 144


class PftLayout(C.Structure):
    """dabgpu_pft_layout_info: how AF packets of one size are cut into PF fragments (pft_layout)"""
    _fields_ = [(f, C.c_int32) for f in ("packet_bytes", "fec", "m", "max_payload", "addr", "chunks", "rs_k", "rs_z", "block_bytes",
                                         "fcount", "plen", "header_bytes", "stream_bytes", "guaranteed_losses")] + \
               [("reserved", C.c_int32 * 2)]


class PftReadEntry(C.Structure):
    """dabgpu_pft_read_entry: one PF fragment byte stream of Context.pft_read_dev (device addresses) or pft_read_host (host
    addresses).  d_out holds pft_read_out_bytes(n_bytes), d_records pft_read_max_records(n_bytes) records."""
    _fields_ = [("d_bytes", C.c_void_p), ("n_bytes", C.c_int32), ("flags", C.c_int32), ("d_state_in", C.c_void_p),
                ("d_state_out", C.c_void_p), ("d_out", C.c_void_p), ("d_records", C.c_void_p), ("d_result", C.c_void_p)]


def pft_layout(packet_bytes, fec=True, m=2, max_payload=1400, addr=False):
    """How AF packets of packet_bytes are cut into PF fragments (dabgpu_pft_layout: host only): with fec, so that any m
    fragments of a packet may be lost, no fragment's payload above max_payload.  -> PftLayout (chunks, rs_k, rs_z, fcount,
    plen, stream_bytes, guaranteed_losses, ...).  DabGpuError for what the rule refuses."""
    info = PftLayout()
    _check(lib().dabgpu_pft_layout(int(packet_bytes), int(bool(fec)), int(m), int(max_payload), int(bool(addr)), C.byref(info)),
           "dabgpu_pft_layout")
    return info


def pft_fragments_host(layout, af, pseq_start=None, source=0, dest=0):
    """AF packets -> PF fragments on HOST memory, serially (dabgpu_pft_fragments_host).  af: uint8 [n_streams][n_packets *
    layout.packet_bytes]; pseq_start: the first packet's Pseq per stream (None: 0).  -> uint8 [n_streams][n_packets *
    layout.stream_bytes]."""
    af = np.ascontiguousarray(af, np.uint8)
    n_streams, n_in = af.shape
    n_packets = n_in // layout.packet_bytes
    if n_packets * layout.packet_bytes != n_in:
        raise ValueError("af must hold whole packets of layout.packet_bytes")
    in_stride, out_stride = (n_in + 15) // 16 * 16, (n_packets * layout.stream_bytes + 15) // 16 * 16
    src, dst = _aligned_bytes(max(n_streams * in_stride, 16)), _aligned_bytes(max(n_streams * out_stride, 16))
    src[:n_streams * in_stride].reshape(n_streams, in_stride)[:, :n_in] = af
    seq = None if pseq_start is None else (C.c_uint32 * max(n_streams, 1))(*[int(v) & 0xFFFFFFFF for v in pseq_start])
    _check(lib().dabgpu_pft_fragments_host(C.byref(layout), n_streams, n_packets, _p(src), in_stride, seq, int(source), int(dest), _p(dst),
                                           out_stride), "dabgpu_pft_fragments_host")
    return dst[:n_streams * out_stride].reshape(n_streams, out_stride)[:, :n_packets * layout.stream_bytes].copy()


def _aligned_bytes(n, fill=0):
    """a uint8 array of n bytes on a 16-byte boundary"""
    raw = np.full(n + 16, fill, np.uint8)
    at = (-raw.ctypes.data) % 16
    return raw[at:at + n]


def pft_read_state_bytes():
    """Bytes of one state record of Context.pft_read_dev / pft_read_host (all zero = a stream that starts)."""
    return int(lib().dabgpu_pft_read_state_bytes())


def pft_read_out_bytes(n_bytes):
    """Bytes one entry can emit in one call: its d_out holds this many."""
    return int(lib().dabgpu_pft_read_out_bytes(int(n_bytes)))


def pft_read_max_records(n_bytes):
    """Records one entry can leave in one call: its d_records holds this many."""
    return int(lib().dabgpu_pft_read_max_records(int(n_bytes)))


def pft_read_host(entries):
    """Context.pft_read_dev on HOST memory (entries: PftReadEntry with host addresses): the same checks and the header's
    serial reader, without a context or a GPU (dabgpu_pft_read_host)."""
    _entries_call("dabgpu_pft_read_host", PftReadEntry, entries)


#: ETI(NI) to IQ (include/dabgpu.h, "ETI(NI) to IQ"): dabgpu_mod_status, one transmission frame's record
MOD_BAD_INPUT, MOD_MISALIGNED = 1, 2
MOD_STATUS_DTYPE = np.dtype([("flags", np.uint32), ("refused", np.uint8), ("reserved", np.uint8, (3,))])
assert MOD_STATUS_DTYPE.itemsize == 8
#: mean_kernel_ms / last_kernel_ms selectors of the modulator: the encoder with its pre-pass, the symbol kernel
WHICH_MOD_ENCODE, WHICH_MOD_SYMBOLS = 8, 9


class ModCfg(C.Structure):
    """dabgpu_mod_cfg: gain, and the transmitter whose identification the null symbol carries (-1, -1: zeros)."""
    _fields_ = [("gain", C.c_float), ("tii_main", C.c_int32), ("tii_sub", C.c_int32), ("reserved", C.c_int32)]


def mod_cfg(**kw):
    c = ModCfg()
    lib().dabgpu_mod_default_cfg(C.byref(c))
    for k, v in kw.items():
        if not hasattr(c, k):
            raise TypeError("dabgpu_mod_cfg has no field " + k)
        setattr(c, k, v)
    return c


def mod_state_bytes():
    return int(lib().dabgpu_mod_state_bytes())


def eti_streams(frame):
    """The stream list of one 6144-byte ETI(NI) frame, read back from its STC (dabgpu_eti_streams_from_frame: host only):
    [EtiStream, ...] in the frame's order, what eti_layout takes.  DabGpuError (ERR_ARG) for a TPL/STL pair that names
    no protection profile."""
    f = np.ascontiguousarray(np.frombuffer(bytes(frame), np.uint8) if isinstance(frame, (bytes, bytearray)) else frame, np.uint8)
    if f.size != ETI_FRAME_BYTES:
        raise ValueError("an ETI(NI) frame is %d bytes, got %d" % (ETI_FRAME_BYTES, f.size))
    arr = (EtiStream * ETI_MAX_STREAMS)()
    n = C.c_int(0)
    _check(lib().dabgpu_eti_streams_from_frame(_p(f.reshape(-1)), arr, C.byref(n)), "dabgpu_eti_streams_from_frame")
    return [EtiStream(arr[k].subchannel_id, arr[k].sc) for k in range(n.value)]


def eti_parse(frame):
    """Check one 6144-byte ETI(NI) frame (sync, lengths, both CRCs; dabgpu_eti_parse: host only) and give its parts:
    dict with err, fct, fp, nst, fl, length, streams [{scid, sad, tpl, stl, data}], fic (96 bytes).  ValueError for a
    malformed frame."""
    f = np.ascontiguousarray(np.frombuffer(bytes(frame), np.uint8) if isinstance(frame, (bytes, bytearray)) else frame, np.uint8)
    if f.size != ETI_FRAME_BYTES:
        raise ValueError("an ETI(NI) frame is %d bytes, got %d" % (ETI_FRAME_BYTES, f.size))
    f = f.reshape(-1)
    info = EtiInfo()
    rc = lib().dabgpu_eti_parse(_p(f), C.byref(info))
    if rc < 0:
        raise DabGpuError(rc, "dabgpu_eti_parse")
    if rc > 0:
        raise ValueError("not a valid ETI(NI) frame: " + ETI_PARSE_ERRORS.get(rc, str(rc)))
    streams = [{"scid": info.scid[k], "sad": info.sad[k], "tpl": info.tpl[k], "stl": info.stl[k],
                "data": f[info.offset[k]:info.offset[k] + 8 * info.stl[k]].copy()} for k in range(info.nst)]
    return {"err": info.err, "fct": info.fct, "fp": info.fp, "mid": info.mid, "nst": info.nst, "fl": info.fl,
            "length": info.length, "header_crc": info.header_crc, "data_crc": info.data_crc,
            "fic": f[info.fic_offset:info.fic_offset + 96].copy(), "streams": streams}


_LIB = None


def load_library(path):
    """Load one build of libdabgpu.so and declare its entry points.  lib() does this for the in-tree library; tools
    that compare builds inside one process (tools/ab_inproc.py) load others and pass them to Context(library=...)."""
    L = C.CDLL(path)
    L.dabgpu_abi_version.argtypes = []
    L.dabgpu_strerror.restype = C.c_char_p
    L.dabgpu_strerror.argtypes = [C.c_int]
    L.dabgpu_get_ofdm_params.argtypes = [C.c_int, C.c_void_p]
    L.dabgpu_get_dab_params.argtypes = [C.c_int, C.c_void_p]
    L.dabgpu_stream.restype = C.c_void_p
    L.dabgpu_stream.argtypes = [C.c_void_p]
    L.dabgpu_destroy.restype = None
    L.dabgpu_destroy.argtypes = [C.c_void_p]
    vp, sz, i = C.c_void_p, C.c_size_t, C.c_int
    L.dabgpu_create.argtypes = [C.POINTER(Cfg), C.POINTER(vp)]
    L.dabgpu_sync.argtypes = [vp]
    L.dabgpu_ofdm_demod_frames_dev.argtypes = [vp, vp, sz, i, vp, vp, vp, vp, vp]
    L.dabgpu_ofdm_demod_frames.argtypes = [vp, vp, sz, i, vp, vp, vp, vp]
    L.dabgpu_ofdm_demod_frames_dd_dev.argtypes = [vp, vp, sz, i, vp, vp, vp, vp]
    L.dabgpu_test_fail_frame_call.argtypes = [vp, i]
    L.dabgpu_fft_symbols_dev.argtypes = [vp, vp, sz, i, vp, vp, vp]
    L.dabgpu_fft_symbols.argtypes = [vp, vp, sz, i, vp, vp]
    L.dabgpu_fic_decode_dev.argtypes = [vp, vp, sz, i, vp, vp, vp]
    L.dabgpu_fic_decode.argtypes = [vp, vp, sz, i, vp, vp]
    L.dabgpu_subchannel_bytes.argtypes = [C.POINTER(Subchannel)]
    L.dabgpu_msc_decode_dev.argtypes = [vp, C.POINTER(Subchannel), vp, sz, i, i, vp, vp, vp, vp]
    L.dabgpu_msc_decode.argtypes = [vp, C.POINTER(Subchannel), vp, sz, i, i, vp, vp, vp]
    L.dabgpu_viterbi_dev.argtypes = [vp, vp, i, vp, i, vp, vp]
    L.dabgpu_viterbi.argtypes = [vp, vp, i, vp, i, vp]
    L.dabgpu_set_timing.argtypes = [vp, i]
    L.dabgpu_dabplus_superframes_dev.argtypes = [vp, vp, sz, i, i, vp, vp, vp]
    L.dabgpu_dabplus_superframes.argtypes = [vp, vp, sz, i, i, vp, vp]
    L.dabgpu_msc_decode_multi_dev.argtypes = [vp, vp, i, vp, sz, i, i, vp, vp, vp, vp]
    L.dabgpu_decode_frames_dev.argtypes = [vp, vp, sz, i, i, vp, vp, vp, i, vp, vp, vp, vp]
    L.dabgpu_decode_frames.argtypes = [vp, vp, sz, i, i, vp, vp, vp, i, vp, vp, vp]
    L.dabgpu_decode_ensembles_dev.argtypes = [vp, vp, sz, i, i, vp, vp, vp, vp, vp, vp, vp, vp]
    L.dabgpu_fig_subchannels.argtypes = [vp, vp, i, vp, i, C.POINTER(C.c_int)]
    L.dabgpu_fig_audio_components.argtypes = [vp, vp, i, vp, i, C.POINTER(C.c_int)]
    L.dabgpu_dabplus_follow_dev.argtypes = [vp, C.POINTER(DabplusEntry), i, i, vp]
    L.dabgpu_dabplus_carry_bytes.restype = C.c_size_t
    L.dabgpu_dabplus_carry_bytes.argtypes = [i]
    L.dabgpu_pad_state_bytes.restype = C.c_size_t
    L.dabgpu_pad_state_bytes.argtypes = []
    L.dabgpu_pad_labels_dev.argtypes = [vp, C.POINTER(PadEntry), i, vp]
    L.dabgpu_pad_labels_host.argtypes = [C.POINTER(PadEntry), i]
    L.dabgpu_pad_label_utf8.argtypes = [vp, C.c_char_p, i]
    L.dabgpu_mp2_carry_bytes.restype = C.c_size_t
    L.dabgpu_mp2_carry_bytes.argtypes = [i]
    L.dabgpu_mp2_follow_dev.argtypes = [vp, C.POINTER(Mp2Entry), i, i, vp]
    L.dabgpu_mp2_follow_host.argtypes = [C.POINTER(Mp2Entry), i, i]
    L.dabgpu_mp2_subbands_dev.argtypes = [vp, C.POINTER(Mp2AudioEntry), i, i, vp]
    L.dabgpu_mp2_subbands_host.argtypes = [C.POINTER(Mp2AudioEntry), i, i]
    L.dabgpu_mot_state_bytes.restype = C.c_size_t
    L.dabgpu_mot_state_bytes.argtypes = []
    L.dabgpu_mot_arena_bytes.restype = C.c_size_t
    L.dabgpu_mot_arena_bytes.argtypes = [C.c_size_t]
    L.dabgpu_mot_slides_dev.argtypes = [vp, C.POINTER(MotEntry), i, vp]
    L.dabgpu_mot_slides_host.argtypes = [C.POINTER(MotEntry), i]
    L.dabgpu_mot_header_parse.argtypes = [vp, i, C.POINTER(MotHeader)]
    L.dabgpu_fig_packet_components.argtypes = [vp, vp, i, vp, i, C.POINTER(C.c_int)]
    L.dabgpu_packet_state_bytes.restype = C.c_size_t
    L.dabgpu_packet_state_bytes.argtypes = []
    L.dabgpu_packet_slides_dev.argtypes = [vp, C.POINTER(PacketEntry), i, i, vp]
    L.dabgpu_packet_slides_host.argtypes = [C.POINTER(PacketEntry), i, i]
    L.dabgpu_packet_carousel_state_bytes.restype = C.c_size_t
    L.dabgpu_packet_carousel_state_bytes.argtypes = []
    L.dabgpu_packet_carousel_arena_bytes.restype = C.c_size_t
    L.dabgpu_packet_carousel_arena_bytes.argtypes = [i, i, i]
    L.dabgpu_packet_carousel_dev.argtypes = [vp, C.POINTER(PacketCarouselEntry), i, i, vp]
    L.dabgpu_packet_carousel_host.argtypes = [C.POINTER(PacketCarouselEntry), i, i]
    L.dabgpu_packet_groups_state_bytes.restype = C.c_size_t
    L.dabgpu_packet_groups_state_bytes.argtypes = []
    L.dabgpu_packet_groups_chunk.argtypes = []
    L.dabgpu_packet_groups_dev.argtypes = [vp, C.POINTER(PacketGroupsEntry), i, i, vp]
    L.dabgpu_packet_groups_host.argtypes = [C.POINTER(PacketGroupsEntry), i, i]
    L.dabgpu_eti_read_state_bytes.restype = C.c_size_t
    L.dabgpu_eti_read_state_bytes.argtypes = []
    L.dabgpu_eti_read_dev.argtypes = [vp, C.POINTER(EtiReadEntry), i, vp]
    L.dabgpu_eti_read_host.argtypes = [C.POINTER(EtiReadEntry), i]
    L.dabgpu_edi_packet_bytes.argtypes = [C.POINTER(EtiPlan)]
    L.dabgpu_edi_frames_dev.argtypes = [vp, C.POINTER(EtiPlan), i, i, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp, vp]
    L.dabgpu_edi_parse.argtypes = [vp, sz, C.POINTER(EdiInfo)]
    L.dabgpu_edi_streams_from_packet.argtypes = [vp, sz, vp, C.POINTER(C.c_int)]
    L.dabgpu_edi_read_state_bytes.restype = C.c_size_t
    L.dabgpu_edi_read_state_bytes.argtypes = []
    L.dabgpu_edi_read_max_rows.argtypes = [i, C.POINTER(EtiPlan)]
    L.dabgpu_edi_read_host.argtypes = [C.POINTER(EtiReadEntry), i]
    L.dabgpu_edi_read_dev.argtypes = [vp, C.POINTER(EtiReadEntry), i, vp]
    L.dabgpu_pft_layout.argtypes = [i, i, i, i, i, C.POINTER(PftLayout)]
    L.dabgpu_pft_fragments_dev.argtypes = [vp, C.POINTER(PftLayout), i, i, vp, sz, vp, C.c_uint32, C.c_uint32, vp, sz, vp]
    L.dabgpu_pft_fragments_host.argtypes = [C.POINTER(PftLayout), i, i, vp, sz, vp, C.c_uint32, C.c_uint32, vp, sz]
    for fn in (L.dabgpu_pft_read_state_bytes, L.dabgpu_pft_read_out_bytes):
        fn.restype = C.c_size_t
    L.dabgpu_pft_read_state_bytes.argtypes = []
    L.dabgpu_pft_read_out_bytes.argtypes = [i]
    L.dabgpu_pft_read_max_records.argtypes = [i]
    L.dabgpu_pft_read_host.argtypes = [C.POINTER(PftReadEntry), i]
    L.dabgpu_pft_read_dev.argtypes = [vp, C.POINTER(PftReadEntry), i, vp]
    L.dabgpu_fig_user_applications.argtypes = [vp, vp, i, vp, i, C.POINTER(C.c_int)]
    L.dabgpu_mot_directory_parse.argtypes = [vp, i, vp, vp, i, C.POINTER(C.c_int)]
    L.dabgpu_fig_stream_components.argtypes = [vp, vp, i, vp, i, C.POINTER(C.c_int)]
    L.dabgpu_ts_programs.argtypes = [vp, i, C.POINTER(TsInfo)]
    L.dabgpu_dmb_state_bytes.restype = C.c_size_t
    L.dabgpu_dmb_state_bytes.argtypes = []
    L.dabgpu_dmb_max_packets.argtypes = [i, i]
    L.dabgpu_dmb_state_census.argtypes = [vp, i, vp]
    L.dabgpu_dmb_follow_dev.argtypes = [vp, C.POINTER(DmbEntry), i, i, vp]
    L.dabgpu_dmb_follow_host.argtypes = [C.POINTER(DmbEntry), i, i]
    L.dabgpu_packet_fec_state_bytes.restype = C.c_size_t
    L.dabgpu_packet_fec_state_bytes.argtypes = [i]
    L.dabgpu_packet_fec_delay.argtypes = [i]
    L.dabgpu_packet_fec_dev.argtypes = [vp, C.POINTER(PacketFecEntry), i, i, vp]
    L.dabgpu_packet_fec_host.argtypes = [C.POINTER(PacketFecEntry), i, i]
    L.dabgpu_packet_fec_erasures_dev.argtypes = [vp, C.POINTER(PacketFecErasureEntry), i, i, vp]
    L.dabgpu_packet_fec_erasures_host.argtypes = [C.POINTER(PacketFecErasureEntry), i, i]
    L.dabgpu_decode_stream_frames.argtypes = [vp, vp, sz, i, vp, vp, vp, i, vp]
    L.dabgpu_decode_stream_reset.argtypes = [vp]
    L.dabgpu_streams_reset.argtypes = [vp, i]
    L.dabgpu_stream_states.restype = C.c_void_p
    L.dabgpu_stream_states.argtypes = [vp]
    L.dabgpu_set_stream_offsets.argtypes = [vp, i, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.dabgpu_ofdm_demod_streams_dev.argtypes = [vp, vp, sz, i, i, C.c_float, vp, vp, vp, vp]
    L.dabgpu_ofdm_demod_streams.argtypes = [vp, vp, sz, i, i, C.c_float, vp, vp, vp]
    L.dabgpu_get_stats.argtypes = [vp, i, C.POINTER(Stats)]
    L.dabgpu_sync_prs_dev.argtypes = [vp, vp, sz, i, vp, i, vp, vp]
    L.dabgpu_sync_prs.argtypes = [vp, vp, sz, i, vp, i, vp]
    L.dabgpu_ofdm_set_soft_selection.argtypes = [vp, vp, i]
    L.dabgpu_soft_selection.argtypes = [vp, i, i, vp, i]
    L.dabgpu_uep_subchannel.argtypes = [i, i, C.POINTER(Subchannel)]
    L.dabgpu_host_alloc.restype = C.c_void_p
    L.dabgpu_host_alloc.argtypes = [sz]
    L.dabgpu_host_free.restype = None
    L.dabgpu_host_free.argtypes = [C.c_void_p]
    L.dabgpu_acquire_default_cfg.restype = None
    L.dabgpu_acquire_default_cfg.argtypes = [C.POINTER(AcquireCfg)]
    L.dabgpu_acquire_dev.argtypes = [vp, vp, sz, i, C.c_int64, C.POINTER(AcquireCfg), i, vp, vp, vp]
    L.dabgpu_acquire.argtypes = [vp, vp, sz, i, C.c_int64, C.POINTER(AcquireCfg), i, vp, vp]
    L.dabgpu_ofdm_demod_acquired_dev.argtypes = [vp, vp, sz, i, i, vp, vp, vp, vp, vp]
    L.dabgpu_last_kernel_ms.argtypes = [vp, i, C.POINTER(C.c_float)]
    L.dabgpu_mean_kernel_ms.argtypes = [vp, i, C.POINTER(C.c_float), C.POINTER(C.c_int)]
    L.dabgpu_alloc_frame_buffers.argtypes = [vp, i, sz, i, C.POINTER(vp), C.POINTER(vp), C.POINTER(PlacementReport)]
    L.dabgpu_free_frame_buffers.argtypes = [vp, vp, vp]
    L.dabgpu_mover_frames_dev.argtypes = [vp, vp, sz, i, vp, i, vp]
    L.dabgpu_pipe_open.argtypes = [vp, i, i, sz]
    L.dabgpu_pipe_submit.argtypes = [vp, vp, i, i, vp, C.c_float, vp, i, vp, vp, vp, vp, C.POINTER(C.c_int64)]
    L.dabgpu_pipe_wait.argtypes = [vp, C.c_int64]
    L.dabgpu_pipe_reset.argtypes = [vp]
    L.dabgpu_pipe_close.argtypes = [vp]
    L.dabgpu_set_stream_loop.argtypes = [vp, C.c_float, C.c_float, i]
    L.dabgpu_set_loop_gate.argtypes = [vp, C.c_float]
    L.dabgpu_set_iq_format.argtypes = [vp, i]
    L.dabgpu_get_iq_format.argtypes = [vp]
    L.dabgpu_track_default_cfg.restype = None
    L.dabgpu_track_default_cfg.argtypes = [C.POINTER(TrackCfg)]
    L.dabgpu_track_start_dev.argtypes = [vp, vp, vp, i, i, C.c_int64, i, vp]
    L.dabgpu_ofdm_demod_tracked_dev.argtypes = [vp, vp, sz, i, C.c_int64, i, C.c_int64, C.POINTER(TrackCfg), vp, vp, vp, vp, vp, vp]
    L.dabgpu_ofdm_demod_stream_frame.argtypes = [vp, i, vp, i, C.POINTER(TrackCfg), vp, vp, C.POINTER(FrameResult)]
    L.dabgpu_get_prs_reference.argtypes = [i, vp, i]
    L.dabgpu_get_mapper_reference.argtypes = [vp, i, i]
    L.dabgpu_mer_dev.argtypes = [vp, vp, sz, i, i, i, vp, vp]
    L.dabgpu_channel_ber_dev.argtypes = [vp, vp, sz, i, i, vp, vp, vp, i, vp, vp, vp, vp]
    L.dabgpu_decode_stream_frames_quality.argtypes = [vp, vp, sz, i, vp, vp, vp, i, vp, vp, vp, vp]
    L.dabgpu_tii_default_cfg.restype = None
    L.dabgpu_tii_default_cfg.argtypes = [C.POINTER(TiiCfg)]
    L.dabgpu_tii_pattern.argtypes = [i]
    L.dabgpu_tii_frames_dev.argtypes = [vp, vp, sz, i, i, vp, vp, vp, vp]
    L.dabgpu_tii_acquired_dev.argtypes = [vp, vp, sz, i, i, vp, i, vp, vp, vp]
    L.dabgpu_tii_decode.argtypes = [vp, C.POINTER(TiiCfg), vp, i]
    L.dabgpu_cir_default_cfg.restype = None
    L.dabgpu_cir_default_cfg.argtypes = [C.POINTER(CirCfg)]
    L.dabgpu_cir_frames_dev.argtypes = [vp, vp, sz, i, i, vp, vp, vp, vp]
    L.dabgpu_cir_acquired_dev.argtypes = [vp, vp, sz, i, i, vp, i, vp, vp, vp]
    L.dabgpu_cir_analyse.argtypes = [vp, C.POINTER(CirCfg), vp, vp, i]
    L.dabgpu_eti_layout.argtypes = [vp, i, C.POINTER(EtiPlan)]
    L.dabgpu_eti_history_bytes.restype = C.c_size_t
    L.dabgpu_eti_history_bytes.argtypes = []
    L.dabgpu_eti_frames_dev.argtypes = [vp, C.POINTER(EtiPlan), i, i, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.dabgpu_eti_parse.argtypes = [vp, C.POINTER(EtiInfo)]
    L.dabgpu_eti_streams_from_frame.argtypes = [vp, vp, C.POINTER(C.c_int)]
    L.dabgpu_mod_default_cfg.restype = None
    L.dabgpu_mod_default_cfg.argtypes = [C.POINTER(ModCfg)]
    L.dabgpu_mod_state_bytes.restype = C.c_size_t
    L.dabgpu_mod_state_bytes.argtypes = []
    L.dabgpu_modulate_eti_dev.argtypes = [vp, C.POINTER(EtiPlan), vp, C.POINTER(ModCfg), i, i, vp, vp, vp, vp, sz, vp, vp]
    return L


def lib():
    """Load libdabgpu.so (raises if it has not been built -- there is no fallback)."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("libdabgpu.so not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "or `make -C sdrplusplus-dab-radio-plugin_amd/csrc` (expected %s)" % LIB_PATH)
        try:
            # share the HIP runtime torch already loaded (same SONAME libamdhip64.so.7)
            import torch  # noqa: F401
        except Exception:
            pass
        _LIB = load_library(LIB_PATH)
    return _LIB


def strerror(status):
    return lib().dabgpu_strerror(C.c_int(status)).decode()


def _check(rc, what):
    if rc != 0:
        raise DabGpuError(rc, what)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _entries_call(name, kind, entries, *args, ctx=None):
    """The library's call `name` on a list of entries: name(entries, n, *args), or with a Context name(handle, entries, n, *args) of
    the library that context loaded.  `entries` goes as an array of `kind`, at least one element long (an empty list still passes
    an address); raises DabGpuError for a status other than DABGPU_OK."""
    n = len(entries)
    arr = (kind * max(n, 1))(*entries)
    if ctx is None:
        rc = getattr(lib(), name)(arr, n, *args)
    else:
        rc = getattr(ctx._lib, name)(ctx._h, arr, n, *args)
    _check(rc, name)


def _fib_batch(fib, crc_ok):
    """The arguments of the dabgpu_fig_* calls: fib [n_frames][12][32] and crc_ok [n_frames][12] as contiguous uint8 ->
    (fib, crc_ok, n_frames)."""
    fib = np.ascontiguousarray(fib, np.uint8)
    crc_ok = np.ascontiguousarray(crc_ok, np.uint8)
    n_frames = fib.size // (12 * 32)
    if fib.size != n_frames * 12 * 32 or crc_ok.size != n_frames * 12:
        raise ValueError("fib must be [n_frames][12][32] and crc_ok [n_frames][12]")
    return fib, crc_ok, n_frames


# ------------------------------------------------------------------ tables (no GPU needed)
def get_ofdm_params(mode=1):
    p = OfdmParams()
    _check(lib().dabgpu_get_ofdm_params(C.c_int(mode), C.byref(p)), "dabgpu_get_ofdm_params")
    return p


def get_dab_params(mode=1):
    p = DabParams()
    _check(lib().dabgpu_get_dab_params(C.c_int(mode), C.byref(p)), "dabgpu_get_dab_params")
    return p


def get_prs_reference(mode=1):
    out = np.zeros(2 * NB_FFT, np.float32)
    _check(lib().dabgpu_get_prs_reference(mode, _p(out), NB_FFT), "dabgpu_get_prs_reference")
    return out.view(np.complex64)


def get_mapper_reference():
    out = np.zeros(NB_CARRIERS, np.int32)
    _check(lib().dabgpu_get_mapper_reference(_p(out), NB_CARRIERS, NB_FFT), "dabgpu_get_mapper_reference")
    return out


def subchannel(start_address, bitrate_kbps, level=3, eep_type=0):
    """EEP subchannel descriptor with the length implied by the profile."""
    if eep_type == 0:
        n = bitrate_kbps // 8
        length = {1: 12 * n, 2: 8 * n, 3: 6 * n, 4: 4 * n}[level]
    else:
        n = bitrate_kbps // 32
        length = {1: 27 * n, 2: 21 * n, 3: 18 * n, 4: 15 * n}[level]
    return Subchannel(start_address, length, 0, eep_type, level, bitrate_kbps)


class PinnedArray:
    """numpy view of page-locked host memory from dabgpu_host_alloc (freed by close() / garbage collection)."""

    def __init__(self, shape, dtype):
        self._n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        self._p = lib().dabgpu_host_alloc(self._n)
        if not self._p:
            raise MemoryError("dabgpu_host_alloc(%d)" % self._n)
        buf = (C.c_char * self._n).from_address(self._p)
        self.array = np.frombuffer(buf, dtype=dtype).reshape(shape)

    def close(self):
        if self._p:
            self.array = None
            lib().dabgpu_host_free(self._p)
            self._p = None

    def __del__(self, _finalizing=sys.is_finalizing):   # (bound now: module globals are gone when the interpreter ends)
        try:
            if _finalizing():                    # the HIP runtime may be gone already: the process is about to return it all
                return
            self.close()
        except Exception:
            pass


def device_tensor(torch, address, shape, dtype, device):
    """A torch tensor over device memory this library (or anybody else) owns -- no copy, no ownership: the memory must
    outlive the tensor.  Goes through __cuda_array_interface__, which torch's HIP build honours."""
    typestr = {torch.int8: "|i1", torch.uint8: "|u1", torch.float32: "<f4", torch.int32: "<i4", torch.complex64: "<c8"}[dtype]

    class _Span:
        pass
    span = _Span()
    span.__cuda_array_interface__ = {"shape": tuple(int(x) for x in shape), "typestr": typestr, "data": (int(address), False), "version": 2}
    return torch.as_tensor(span, device=device)


def uep_subchannel(table_index, start_address):
    """UEP subchannel descriptor from the protection-profile table index (FIG 0/1 short form)."""
    sc = Subchannel()
    _check(lib().dabgpu_uep_subchannel(table_index, start_address, C.byref(sc)), "dabgpu_uep_subchannel")
    return sc


def fig_subchannels(fib, crc_ok, max_out=64):
    """The sub-channel list one ensemble announces (FIG 0/1) in its CRC-clean FIBs, sorted by start address: fib
    [n_frames][12][32] uint8, crc_ok [n_frames][12] -> list of Subchannel (no GPU needed)."""
    fib, crc_ok, n_frames = _fib_batch(fib, crc_ok)
    arr = (Subchannel * max(max_out, 1))()
    n = C.c_int(0)
    _check(lib().dabgpu_fig_subchannels(_p(fib), _p(crc_ok), n_frames, arr, max_out, C.byref(n)), "dabgpu_fig_subchannels")
    return [Subchannel(a.start_address, a.length, a.is_uep, a.eep_type, a.protection_level, a.bitrate_kbps) for a in arr[:n.value]]


def fig_audio_components(fib, crc_ok, max_out=64):
    """The MSC stream audio components one ensemble announces (FIG 0/2 joined to FIG 0/1) in its CRC-clean FIBs, each
    sub-channel once, sorted by start address: fib [n_frames][12][32] uint8, crc_ok [n_frames][12] -> list of
    AudioComponent (ascty 0 = DAB, 63 = DAB+; no GPU needed)."""
    fib, crc_ok, n_frames = _fib_batch(fib, crc_ok)
    arr = (AudioComponent * max(max_out, 1))()
    n = C.c_int(0)
    _check(lib().dabgpu_fig_audio_components(_p(fib), _p(crc_ok), n_frames, arr, max_out, C.byref(n)), "dabgpu_fig_audio_components")
    return [AudioComponent(a.sid, a.subchid, a.start_address, a.ascty, a.primary) for a in arr[:n.value]]


def fig_packet_components(fib, crc_ok, max_out=64):
    """The packet-mode service components one ensemble announces (FIG 0/2 TMId 3 joined to FIG 0/3, FIG 0/1 and FIG 0/14) in
    its CRC-clean FIBs, each (sub-channel, packet address) once, sorted by (start address, packet address): fib
    [n_frames][12][32] uint8, crc_ok [n_frames][12] -> list of PacketComponent (dscty 60 = MOT; no GPU needed)."""
    fib, crc_ok, n_frames = _fib_batch(fib, crc_ok)
    arr = (PacketComponent * max(max_out, 1))()
    n = C.c_int(0)
    _check(lib().dabgpu_fig_packet_components(_p(fib), _p(crc_ok), n_frames, arr, max_out, C.byref(n)), "dabgpu_fig_packet_components")
    return [PacketComponent(a.sid, a.scid, a.subchid, a.start_address, a.packet_address, a.dscty, a.dg_flag, a.fec_scheme, a.primary)
            for a in arr[:n.value]]


def fig_user_applications(fib, crc_ok, max_out=64):
    """The user applications one ensemble announces (FIG 0/13) in its CRC-clean FIBs, each (SId, SCIdS, type) once, joined
    through FIG 0/8 (and FIG 0/3 for packet mode) to its component, sorted by (sid, scids, ua_type): fib
    [n_frames][12][32] uint8, crc_ok [n_frames][12] -> a USER_APPLICATION_DTYPE array (no GPU needed)."""
    fib, crc_ok, n_frames = _fib_batch(fib, crc_ok)
    out = np.zeros(max(max_out, 1), USER_APPLICATION_DTYPE)
    n = C.c_int(0)
    _check(lib().dabgpu_fig_user_applications(_p(fib), _p(crc_ok), n_frames, _p(out), max_out, C.byref(n)), "dabgpu_fig_user_applications")
    return out[:n.value].copy()


def packet_groups_state_bytes():
    """Bytes of one state record of Context.packet_groups_dev / packet_groups_host (all zero = a fresh start)."""
    return int(lib().dabgpu_packet_groups_state_bytes())


def packet_groups_chunk():
    """The followed packets the kernel of Context.packet_groups_dev takes at a time: its seams lie at multiples of this."""
    return int(lib().dabgpu_packet_groups_chunk())


def packet_groups_host(entries, n_cifs):
    """Context.packet_groups_dev on HOST memory (entries: PacketGroupsEntry with host addresses): the same checks and the same
    code, include/dabgpu_data_groups.h; no context, no GPU."""
    _entries_call("dabgpu_packet_groups_host", PacketGroupsEntry, entries, n_cifs)


def packet_state_bytes():
    """Bytes of one state record of Context.packet_slides_dev / packet_slides_host (all zero = a fresh start)."""
    return int(lib().dabgpu_packet_state_bytes())


def packet_carousel_state_bytes():
    """Bytes of one state record of Context.packet_carousel_dev / packet_carousel_host (all zero = a fresh start)."""
    return int(lib().dabgpu_packet_carousel_state_bytes())


def packet_carousel_arena_bytes(directory_capacity, assemblies, object_capacity):
    """The smallest arena of Context.packet_carousel_dev / packet_carousel_host for these three sizes."""
    n = int(lib().dabgpu_packet_carousel_arena_bytes(int(directory_capacity), int(assemblies), int(object_capacity)))
    if n == 0:
        raise ValueError("sizes outside their ranges: %r" % ((directory_capacity, assemblies, object_capacity),))
    return n


def packet_carousel_host(entries, n_cifs):
    """Context.packet_carousel_dev on HOST memory (entries: PacketCarouselEntry with host addresses): the same checks and the
    same code, include/dabgpu_mot_carousel.h; no context, no GPU."""
    _entries_call("dabgpu_packet_carousel_host", PacketCarouselEntry, entries, n_cifs)


def mot_directory_parse(directory, max_objects=256):
    """A MOT directory (the bytes d_directory holds) -> (info, objects): a MOT_DIRECTORY_DTYPE record and a
    MOT_DIRECTORY_OBJECT_DTYPE array, one per listed object; directory[header_offset:][:header_bytes] is what
    mot_header_parse takes.  Raises for a directory the check refuses (no GPU needed)."""
    d = np.ascontiguousarray(np.frombuffer(bytes(directory), np.uint8))
    info = np.zeros(1, MOT_DIRECTORY_DTYPE)
    out = np.zeros(max(max_objects, 1), MOT_DIRECTORY_OBJECT_DTYPE)
    n = C.c_int(0)
    _check(lib().dabgpu_mot_directory_parse(_p(d) if d.size else _p(np.zeros(1, np.uint8)), d.size, _p(info), _p(out), max_objects,
                                            C.byref(n)), "dabgpu_mot_directory_parse")
    return info[0], out[:n.value].copy()


#: T-DMB stream-mode sub-channels (include/dabgpu.h, "T-DMB"; include/dabgpu_dmb.h)
DSCTY_MPEG2_TS = 24
DMB_TS_BYTES, DMB_CENSUS = 188, 32
DMB_AS_RECEIVED, DMB_CORRECTED, DMB_UNCORRECTABLE = 0, 1, 2
DMB_EXEMPT = 1
#: dabgpu_dmb_record: one emitted TS packet
DMB_RECORD_DTYPE = np.dtype([("status", np.uint8), ("corrected_data", np.uint8), ("corrected_parity", np.uint8), ("byte3", np.uint8),
                             ("pid", np.uint16), ("flags", np.uint8), ("reserved", np.uint8), ("position", np.uint32),
                             ("reserved2", np.uint32)])
assert DMB_RECORD_DTYPE.itemsize == 16
#: dabgpu_dmb_result: what one entry of dmb_follow_dev / dmb_follow_host counted in one call, and where the stream stands
DMB_COUNTERS = ("cifs", "bytes", "sync_hits", "locks", "lock_losses", "packets_emitted", "packets_clean", "packets_corrected",
                "packets_uncorrectable", "packets_dropped", "bytes_corrected", "parity_bytes_corrected", "discontinuities",
                "duplicates")
DMB_RESULT_DTYPE = np.dtype([(n, np.int32) for n in DMB_COUNTERS + ("locked", "phase", "pids", "pids_overflowed", "packets_deferred",
                                                                   "packets_lost")])
DMB_DEFER_ROOM = 64
assert DMB_RESULT_DTYPE.itemsize == 80
#: dabgpu_dmb_census_entry
DMB_CENSUS_DTYPE = np.dtype([("pid", np.uint16), ("reserved", np.uint16), ("packets", np.uint32), ("discontinuities", np.uint32),
                             ("duplicates", np.uint32), ("scrambled", np.uint32)])
assert DMB_CENSUS_DTYPE.itemsize == 20


def dmb_state_bytes():
    """Bytes of one state record of Context.dmb_follow_dev / dmb_follow_host (NULL or all zero = a fresh start)."""
    return int(lib().dabgpu_dmb_state_bytes())


def dmb_max_packets(bitrate, n_cifs):
    """ceil(3 * bitrate * n_cifs / 204) + DMB_DEFER_ROOM: the most TS packets a call of n_cifs frames can emit -- what it completes and
    what an earlier call deferred; with this much room in d_ts / d_records nothing is ever deferred."""
    n = int(lib().dabgpu_dmb_max_packets(int(bitrate), int(n_cifs)))
    if n < 0:
        raise ValueError("not a stream-mode bit rate or frame count: %r, %r" % (bitrate, n_cifs))
    return n


def dmb_state_census(state, bitrate):
    """The PID census of a state record on the host (uint8 array of dmb_state_bytes(), or None) -> DMB_CENSUS_DTYPE array,
    the first 32 distinct PIDs in the order they appeared, cumulative counts (dabgpu_dmb_state_census)."""
    out = np.zeros(DMB_CENSUS, DMB_CENSUS_DTYPE)
    st = None if state is None else np.ascontiguousarray(state, np.uint8)
    if st is not None and st.size != dmb_state_bytes():
        raise ValueError("a state record has dmb_state_bytes() bytes")
    n = lib().dabgpu_dmb_state_census(None if st is None else _p(st), int(bitrate), _p(out))
    _check(min(n, 0), "dabgpu_dmb_state_census")
    return out[:n].copy()


def fig_stream_components(fib, crc_ok, max_out=64):
    """The stream-mode data components one ensemble announces (FIG 0/2 TMId 1 joined to FIG 0/1) in its CRC-clean FIBs, each
    sub-channel once, sorted by start address: fib [n_frames][12][32] uint8, crc_ok [n_frames][12] -> list of
    StreamComponent (dscty DSCTY_MPEG2_TS = T-DMB; no GPU needed)."""
    fib, crc_ok, n_frames = _fib_batch(fib, crc_ok)
    arr = (StreamComponent * max(max_out, 1))()
    n = C.c_int(0)
    _check(lib().dabgpu_fig_stream_components(_p(fib), _p(crc_ok), n_frames, arr, max_out, C.byref(n)), "dabgpu_fig_stream_components")
    return [StreamComponent(a.sid, a.subchid, a.start_address, a.dscty, a.primary, a.ca) for a in arr[:n.value]]


def ts_programs(ts):
    """The programmes of TS packets (uint8 [n][188], e.g. what dmb_follow leaves in d_ts): PAT and PMT sections assembled and
    checked (dabgpu_ts_programs: host only) -> TsInfo."""
    ts = np.ascontiguousarray(ts, np.uint8)
    if ts.size % 188:
        raise ValueError("TS packets are 188 bytes")
    info = TsInfo()
    _check(lib().dabgpu_ts_programs(_p(ts) if ts.size else None, ts.size // 188, C.byref(info)), "dabgpu_ts_programs")
    return info


def dmb_follow_host(entries, n_cifs):
    """Context.dmb_follow_dev on HOST memory (entries: DmbEntry with host addresses): the same checks and the serial code of
    include/dabgpu_dmb.h; no context, no GPU."""
    _entries_call("dabgpu_dmb_follow_host", DmbEntry, entries, n_cifs)


def packet_fec_state_bytes(bitrate):
    """Bytes of the state record of Context.packet_fec_dev / packet_fec_host for a sub-channel of this bit rate (NULL or all
    zero = a fresh start)."""
    n = int(lib().dabgpu_packet_fec_state_bytes(int(bitrate)))
    if n == 0:
        raise ValueError("not a packet-mode bit rate: %r" % (bitrate,))
    return n


def packet_fec_delay(bitrate):
    """D = ceil(102 / (bitrate / 8)): the logical frames the output of packet_fec_dev / packet_fec_host lags its input."""
    d = int(lib().dabgpu_packet_fec_delay(int(bitrate)))
    if d < 0:
        raise ValueError("not a packet-mode bit rate: %r" % (bitrate,))
    return d


def packet_fec_host(entries, n_cifs):
    """Context.packet_fec_dev on HOST memory (entries: PacketFecEntry with host addresses): the same checks and the same
    code, include/dabgpu_packet_fec.h; no context, no GPU."""
    _entries_call("dabgpu_packet_fec_host", PacketFecEntry, entries, n_cifs)


def packet_fec_erasures_host(entries, n_cifs):
    """Context.packet_fec_erasures_dev on HOST memory (entries: PacketFecErasureEntry with host addresses): the same checks
    and the same code, include/dabgpu_packet_fec_erasures.h; no context, no GPU."""
    _entries_call("dabgpu_packet_fec_erasures_host", PacketFecErasureEntry, entries, n_cifs)


def packet_slides_host(entries, n_cifs):
    """Context.packet_slides_dev on HOST memory (entries: PacketEntry with host addresses): the same checks and the same
    code, include/dabgpu_packet_walk.h; no context, no GPU."""
    _entries_call("dabgpu_packet_slides_host", PacketEntry, entries, n_cifs)


def dabplus_carry_bytes(bitrate_kbps):
    """Bytes of one carry record of Context.dabplus_follow_dev (0 for a bit rate it refuses)."""
    return int(lib().dabgpu_dabplus_carry_bytes(bitrate_kbps))


def pad_state_bytes():
    """Bytes of one state record of Context.pad_labels_dev / pad_labels_host (all zero = a fresh start)."""
    return int(lib().dabgpu_pad_state_bytes())


def pad_labels_host(entries):
    """Context.pad_labels_dev on HOST memory (entries: PadEntry with host addresses): the same checks and the same walk,
    no context and no GPU."""
    _entries_call("dabgpu_pad_labels_host", PadEntry, entries)


def mp2_carry_bytes(bitrate_kbps):
    """Bytes of one carry record of Context.mp2_follow_dev / mp2_follow_host (0 for a bit rate they refuse)."""
    return int(lib().dabgpu_mp2_carry_bytes(bitrate_kbps))


def mp2_follow_host(entries, n_cifs):
    """Context.mp2_follow_dev on HOST memory (entries: Mp2Entry with host addresses): the same checks and the same code,
    include/dabgpu_mp2_frame.h; no context, no GPU."""
    _entries_call("dabgpu_mp2_follow_host", Mp2Entry, entries, n_cifs)


def mp2_subbands_host(entries, n_cifs):
    """Context.mp2_subbands_dev on HOST memory (entries: Mp2AudioEntry with host addresses): the same checks and the same
    code, include/dabgpu_mp2_audio.h; no context, no GPU."""
    _entries_call("dabgpu_mp2_subbands_host", Mp2AudioEntry, entries, n_cifs)


def pad_label_utf8(label):
    """The text of one PAD_LABEL_DTYPE record as str: charset 15 (UTF-8, validated) and 6 (UCS-2 big-endian); any other
    charset raises DabGpuError with status -5, text that is not valid in its charset -1."""
    rec = np.ascontiguousarray(np.asarray(label, PAD_LABEL_DTYPE).reshape(-1)[:1])
    buf = C.create_string_buffer(400)
    n = lib().dabgpu_pad_label_utf8(rec.ctypes.data, buf, len(buf))
    if n < 0:
        raise DabGpuError(n, "dabgpu_pad_label_utf8")
    return buf.raw[:n].decode("utf-8")


def mot_state_bytes():
    """Bytes of one state record of Context.mot_slides_dev / mot_slides_host (all zero = a fresh start)."""
    return int(lib().dabgpu_mot_state_bytes())


def mot_arena_bytes(body_capacity):
    """Bytes of the smallest arena for slides whose body has up to body_capacity bytes (0: more than the call supports)."""
    return int(lib().dabgpu_mot_arena_bytes(body_capacity))


def mot_slides_host(entries):
    """Context.mot_slides_dev on HOST memory (entries: MotEntry with host addresses): the same checks and the same walk,
    no context and no GPU."""
    _entries_call("dabgpu_mot_slides_host", MotEntry, entries)


def mot_header_parse(header):
    """The MOT header of a slide (bytes) -> dict: the header core, and of the header extension name (bytes), name_charset,
    trigger / expire ("now", the first four bytes as int, or None), category_id, slide_id, category_title, click_through_url,
    alternative_location_url (bytes, None where the parameter is not there), n_params, n_unknown."""
    raw = np.frombuffer(bytes(header), np.uint8)
    out = MotHeader()
    _check(lib().dabgpu_mot_header_parse(raw.ctypes.data if raw.size else None, raw.size, C.byref(out)), "dabgpu_mot_header_parse")
    text = lambda t: None if t.length < 0 else bytes(t.bytes[:t.length])
    when = lambda has, now, t: None if not has else "now" if now else int(t)
    return dict(body_size=out.body_size, header_size=out.header_size, content_type=out.content_type, content_subtype=out.content_subtype,
                n_params=out.n_params, n_unknown=out.n_unknown, name=text(out.name), name_charset=out.name_charset if out.name.length >= 0 else None,
                trigger=when(out.has_trigger, out.trigger_now, out.trigger_time), expire=when(out.has_expire, out.expire_now, out.expire_time),
                category_id=out.category_id if out.has_category else None, slide_id=out.slide_id if out.has_category else None,
                category_title=text(out.category_title), click_through_url=text(out.click_through_url),
                alternative_location_url=text(out.alternative_location_url))


# ------------------------------------------------------------------ context
# Contexts still open when the interpreter ends are closed from an atexit handler -- registered when this module is
# imported, i.e. after torch's own, so it runs BEFORE them -- while the HIP runtime is certainly still there; what the
# garbage collector finds after that is left to the operating system.
_LIVE_CONTEXTS = weakref.WeakSet()


def _close_live_contexts():
    for c in list(_LIVE_CONTEXTS):
        try:
            c.close()
        except Exception:
            pass


atexit.register(_close_live_contexts)


def placement_report_dict(rep, requested=None, final_bytes=None):
    """dabgpu_placement_report as a plain dict, field for field (what bench.py prints as config.buffer_placement and every
    rank's row carries): nothing is decided or measured here."""
    d = {"method": "domain-aware pair" if rep.method == 1 else "plain hipMalloc pair",
         "fallback_reason": None if rep.method == 1 else PLAIN_REASONS.get(rep.fallback_reason, str(rep.fallback_reason)),
         "runtime_error": int(rep.runtime_error), "chunks_taken": int(rep.n_chunks), "chunk_bytes": int(rep.chunk_bytes),
         "chunk_domains": rep.domains.decode(), "domains_seen": int(rep.n_domains),
         "iq_chunks": int(rep.iq_chunks), "soft_chunks": int(rep.soft_chunks),
         "iq_chunk_domains": rep.iq_map.decode(), "soft_chunk_domains": rep.soft_map.decode(),
         "soft_bits_written_beside_same_domain_reads_per_mille": int(rep.conflicts),
         "classify_ms": round(float(rep.classify_ms), 2),
         "pair_over_same_domain": round(float(rep.pair_over_same_domain), 3),
         "setup_peak_bytes": int(rep.setup_peak_bytes)}
    if requested is not None:
        d = dict({"requested": requested}, **d)
    if final_bytes:
        d["setup_peak_over_final_footprint"] = round(rep.setup_peak_bytes / final_bytes, 3)
    return d


class Context:
    """Owns a dabgpu_ctx.  Host-array methods copy in/out and synchronise; *_dev methods take
    raw device addresses (e.g. torch.Tensor.data_ptr()) and a stream handle and only enqueue."""

    def __init__(self, device=0, max_frames=64, flags=0, ofdm_symbol_runs=0, library=None):
        self._h = C.c_void_p()
        self._device = int(device)
        self._lib = library if library is not None else lib()
        cfg = Cfg(device, max_frames, 1, flags, ofdm_symbol_runs)
        _check(self._lib.dabgpu_create(C.byref(cfg), C.byref(self._h)), "dabgpu_create")
        _LIVE_CONTEXTS.add(self)

    def close(self):
        if self._h:
            self._lib.dabgpu_destroy(self._h)
            self._h = C.c_void_p()
        _LIVE_CONTEXTS.discard(self)

    def __del__(self, _finalizing=sys.is_finalizing):
        try:
            if _finalizing():                    # (see _close_live_contexts: contexts are closed before the interpreter goes)
                return
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def stream(self):
        return self._lib.dabgpu_stream(self._h)

    def sync(self):
        _check(self._lib.dabgpu_sync(self._h), "dabgpu_sync")

    def set_timing(self, on):
        _check(self._lib.dabgpu_set_timing(self._h, 1 if on else 0), "dabgpu_set_timing")

    def last_kernel_ms(self, which):
        ms = C.c_float(0)
        _check(self._lib.dabgpu_last_kernel_ms(self._h, which, C.byref(ms)), "dabgpu_last_kernel_ms")
        return ms.value

    def mean_kernel_ms(self, which):
        """(mean ms, launches) of kernel family `which` since set_timing(True) (at most the last 32 launches)."""
        ms, n = C.c_float(0), C.c_int(0)
        _check(self._lib.dabgpu_mean_kernel_ms(self._h, which, C.byref(ms), C.byref(n)), "dabgpu_mean_kernel_ms")
        return ms.value, n.value

    # ---- closed-loop stream call
    def alloc_frame_buffers(self, n_frames, frame_stride=NB_FRAME_SAMPLES, placement=PLACE_PLAIN):
        """Device buffers for [n_frames][frame_stride] cf32 samples and [n_frames][230400] soft bits
        (dabgpu_alloc_frame_buffers): two hipMallocs, or (PLACE_DOMAINS) placed by HBM domain inside 1.5 x their size.
        -> (d_iq, d_soft, PlacementReport): raw device addresses; release with free_frame_buffers."""
        d_iq, d_soft = C.c_void_p(), C.c_void_p()
        rep = PlacementReport()
        _check(self._lib.dabgpu_alloc_frame_buffers(self._h, n_frames, frame_stride, placement, C.byref(d_iq), C.byref(d_soft),
                                                    C.byref(rep)), "dabgpu_alloc_frame_buffers")
        return d_iq.value, d_soft.value, rep

    def test_fail_frame_call(self, nth):
        """Test hook: the nth one-frame call from now on reports DABGPU_ERR_HIP before any launch (0 disarms)."""
        _check(self._lib.dabgpu_test_fail_frame_call(self._h, nth), "dabgpu_test_fail_frame_call")

    def mover_frames_dev(self, d_iq, frame_stride, n_frames, d_soft, with_prefixes=False, stream=None):
        """The front end's loads and stores without its arithmetic (dabgpu_mover_frames_dev); overwrites d_soft."""
        _check(self._lib.dabgpu_mover_frames_dev(self._h, d_iq, frame_stride, n_frames, d_soft, 1 if with_prefixes else 0, stream),
               "dabgpu_mover_frames_dev")

    # ---- host-fed ring
    def pipe_open(self, slots, max_frames, frame_stride=FRAME_USED_SAMPLES):
        _check(self._lib.dabgpu_pipe_open(self._h, slots, max_frames, frame_stride), "dabgpu_pipe_open")

    def pipe_submit(self, iq, n_streams, frames_per_stream, freq_offset, scs, soft, fib, crc_ok, outs, beta=0.9):
        """Enqueue one batch (dabgpu_pipe_submit).  Every array argument is a numpy array (or None for freq_offset / soft)
        that the CALLER keeps alive and untouched until pipe_wait(ticket); page-locked ones (PinnedArray.array) move at the
        link rate.  A ring of integer samples (set_iq_format before pipe_open) takes int16 / int8 / uint8 arrays of shape
        [n, frame_stride, 2] of exactly its format's dtype.  -> ticket"""
        fmt = self.iq_format
        if fmt != IQ_CF32 and (iq.dtype != IQ_DTYPES[fmt] or iq.ndim != 3 or iq.shape[-1] != 2):
            raise ValueError("the ring reads %s samples as [n, frame_stride, 2]; got %s %s" % (IQ_DTYPES[fmt], iq.dtype, iq.shape))
        if fmt == IQ_CF32 and iq.dtype.kind in "iu":
            raise ValueError("the ring reads cf32 samples; set_iq_format before pipe_open for %s" % iq.dtype)
        n = len(scs)
        arr = (Subchannel * max(n, 1))(*scs)
        ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in outs]) if n else None
        t = C.c_int64(-1)
        _check(self._lib.dabgpu_pipe_submit(self._h, iq.ctypes.data, n_streams, frames_per_stream,
                                            None if freq_offset is None else freq_offset.ctypes.data, beta, arr, n,
                                            None if soft is None else soft.ctypes.data, fib.ctypes.data, crc_ok.ctypes.data, ptrs,
                                            C.byref(t)), "dabgpu_pipe_submit")
        return t.value

    def pipe_wait(self, ticket):
        _check(self._lib.dabgpu_pipe_wait(self._h, ticket), "dabgpu_pipe_wait")

    def pipe_reset(self):
        _check(self._lib.dabgpu_pipe_reset(self._h), "dabgpu_pipe_reset")

    def pipe_close(self):
        _check(self._lib.dabgpu_pipe_close(self._h), "dabgpu_pipe_close")

    def free_frame_buffers(self, d_iq, d_soft):
        _check(self._lib.dabgpu_free_frame_buffers(self._h, d_iq, d_soft), "dabgpu_free_frame_buffers")

    def streams_reset(self, n_streams):
        _check(self._lib.dabgpu_streams_reset(self._h, n_streams), "dabgpu_streams_reset")

    @property
    def stream_states_ptr(self):
        return self._lib.dabgpu_stream_states(self._h)

    def set_stream_offsets(self, stream, fine=None, coarse=None):
        f = None if fine is None else C.byref(C.c_float(fine))
        c = None if coarse is None else C.byref(C.c_float(coarse))
        _check(self._lib.dabgpu_set_stream_offsets(self._h, stream, f, c), "dabgpu_set_stream_offsets")

    def get_stats(self, stream):
        st = Stats()
        _check(self._lib.dabgpu_get_stats(self._h, stream, C.byref(st)), "dabgpu_get_stats")
        return st

    def set_stream_loop(self, signal_update_beta=0.95, thr_null_start=0.35, decision_directed=False):
        _check(self._lib.dabgpu_set_stream_loop(self._h, signal_update_beta, thr_null_start, int(bool(decision_directed))),
               "dabgpu_set_stream_loop")

    def stream_states_host(self, n_streams):
        """The first n_streams stream states as a numpy record array (STREAM_STATE_DTYPE), read back after waiting for the
        context stream.  The caller syncs whatever other stream the last stream call ran on."""
        import torch
        self.sync()
        t = device_tensor(torch, self.stream_states_ptr, (n_streams * 64,), torch.uint8, torch.device("cuda", self._device))
        torch.cuda.synchronize()
        return t.cpu().numpy().view(STREAM_STATE_DTYPE).copy()

    def set_iq_format(self, fmt):
        """Sample format the device-pointer calls and a ring opened after this read (IQ_CF32 / IQ_CS16 / IQ_CS8 / IQ_CU8;
        dabgpu_set_iq_format).  The outputs are bit for bit the cf32 path's on float32 copies of the same values (cu8:
        u - 127.5).  Refused (DabGpuError, ERR_ARG) for an unknown value or while a ring is open."""
        _check(self._lib.dabgpu_set_iq_format(self._h, int(fmt)), "dabgpu_set_iq_format")

    @property
    def iq_format(self):
        return self._lib.dabgpu_get_iq_format(self._h)

    def set_loop_gate(self, dd_gate):
        _check(self._lib.dabgpu_set_loop_gate(self._h, dd_gate), "dabgpu_set_loop_gate")

    def track_start_dev(self, d_frames, d_counts, n_streams, max_frames, advance, stream=None, only_lost=False):
        _check(self._lib.dabgpu_track_start_dev(self._h, d_frames, d_counts, n_streams, max_frames, advance, int(bool(only_lost)),
                                            stream), "dabgpu_track_start_dev")

    def ofdm_demod_tracked_dev(self, d_iq, stream_stride, n_streams, n_samples, max_frames, advance, d_soft, d_frames, d_counts,
                               cfg=None, d_cyc=None, d_dqpsk=None, stream=None):
        _check(self._lib.dabgpu_ofdm_demod_tracked_dev(self._h, d_iq, stream_stride, n_streams, n_samples, max_frames, advance,
                                                   None if cfg is None else C.byref(cfg), d_soft, d_cyc, d_dqpsk, d_frames,
                                                   d_counts, stream), "dabgpu_ofdm_demod_tracked_dev")

    def ofdm_demod_stream_frame(self, iq, stream=0, acquiring=False, cfg=None, want_dqpsk=False):
        """One frame (76*2552 cf32, host) of stream `stream` in one call -> soft [230400], FrameResult, dqpsk or None."""
        iq = np.ascontiguousarray(iq, np.complex64).reshape(-1)
        assert iq.size >= FRAME_USED_SAMPLES
        soft = np.zeros(NB_FRAME_BITS, np.int8)
        dq = np.zeros((NB_SYMBOLS - 1, NB_CARRIERS), np.complex64) if want_dqpsk else None
        res = FrameResult()
        _check(self._lib.dabgpu_ofdm_demod_stream_frame(self._h, stream, _p(iq), int(bool(acquiring)),
                                                    None if cfg is None else C.byref(cfg), _p(soft), _p(dq), C.byref(res)),
               "dabgpu_ofdm_demod_stream_frame")
        return soft, res, dq

    def ofdm_demod_streams(self, iq, n_streams, beta=0.9, want_cyc=False, soft=None):
        """iq: complex64 [n_streams*frames_per_stream][>=76*2552]; uses and updates the context's stream states.
        `soft` may be an existing array (selected ranges only are overwritten when a selection is active)."""
        iq = np.ascontiguousarray(iq, np.complex64)
        n_frames, stride = iq.shape
        if soft is None:
            soft = np.zeros((n_frames, NB_FRAME_BITS), np.int8)
        cyc = np.zeros((n_frames, NB_SYMBOLS), np.complex64) if want_cyc else None
        _check(self._lib.dabgpu_ofdm_demod_streams(self._h, _p(iq), stride, n_streams, n_frames // n_streams, beta, _p(soft),
                                               _p(cyc), None), "dabgpu_ofdm_demod_streams")
        return soft, cyc

    def ofdm_demod_streams_dev(self, d_iq, frame_stride, n_streams, frames_per_stream, beta, d_soft, d_cyc=None,
                               d_dqpsk=None, stream=None):
        _check(self._lib.dabgpu_ofdm_demod_streams_dev(self._h, d_iq, frame_stride, n_streams, frames_per_stream, beta, d_soft,
                                                   d_cyc, d_dqpsk, stream), "dabgpu_ofdm_demod_streams_dev")

    def decode_frames(self, soft, n_streams, scs, history_in=None, want_history=False):
        """Host arrays: FIC + sub-channels `scs` of soft [n_streams*frames_per_stream][230400] in one call
        (dabgpu_decode_frames).  -> fib, crc_ok, [out_i], [history_out_i] (or None)"""
        soft = np.ascontiguousarray(soft, np.int8)
        n_frames, stride = soft.shape
        fps = n_frames // n_streams
        n = len(scs)
        arr = (Subchannel * max(n, 1))(*scs)
        fib = np.zeros((n_frames, 12, 32), np.uint8)
        ok = np.zeros((n_frames, 12), np.uint8)
        outs = []
        for sc in scs:
            nb = self._lib.dabgpu_subchannel_bytes(C.byref(sc))
            _check(min(nb, 0), "dabgpu_subchannel_bytes")
            outs.append(np.zeros((n_streams, fps * 4, nb), np.uint8))
        his = [None if history_in is None or history_in[k] is None else np.ascontiguousarray(history_in[k], np.int8)
               for k in range(n)]
        hos = [np.zeros((n_streams, 15, sc.length * 64), np.int8) if want_history else None for sc in scs]

        def ptrs(lst):
            if n == 0:
                return None
            return (C.c_void_p * n)(*[None if a is None else a.ctypes.data for a in lst])
        _check(self._lib.dabgpu_decode_frames(self._h, _p(soft), stride, n_streams, fps, _p(fib), _p(ok), arr, n, ptrs(his),
                                          ptrs(hos), ptrs(outs)), "dabgpu_decode_frames")
        return fib, ok, outs, (hos if want_history else None)

    def decode_stream_frames(self, soft, scs, quality=False):
        """Consecutive frames of one stream; the de-interleaver state stays in the context.  -> fib, crc_ok, [out_i]
        quality=True (dabgpu_decode_stream_frames_quality): -> fib, crc_ok, [out_i], fic_ber [n_frames][4],
        [msc_ber_i [n_frames*4]] (BER_DTYPE), mer [n_frames] (MER_DTYPE, all 75 symbols)"""
        soft = np.ascontiguousarray(soft, np.int8)
        n_frames, stride = soft.shape
        n = len(scs)
        arr = (Subchannel * max(n, 1))(*scs)
        fib = np.zeros((n_frames, 12, 32), np.uint8)
        ok = np.zeros((n_frames, 12), np.uint8)
        outs = []
        for sc in scs:
            nb = self._lib.dabgpu_subchannel_bytes(C.byref(sc))
            _check(min(nb, 0), "dabgpu_subchannel_bytes")
            outs.append(np.zeros((1, n_frames * 4, nb), np.uint8))
        ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in outs]) if n else None
        if not quality:
            _check(self._lib.dabgpu_decode_stream_frames(self._h, _p(soft), stride, n_frames, _p(fib), _p(ok), arr, n, ptrs),
                   "dabgpu_decode_stream_frames")
            return fib, ok, outs
        fic_ber = np.zeros((n_frames, 4), BER_DTYPE)
        msc_ber = [np.zeros(n_frames * 4, BER_DTYPE) for _ in range(n)]
        mer = np.zeros(n_frames, MER_DTYPE)
        bptrs = (C.c_void_p * n)(*[a.ctypes.data for a in msc_ber]) if n else None
        _check(self._lib.dabgpu_decode_stream_frames_quality(self._h, _p(soft), stride, n_frames, _p(fib), _p(ok), arr, n, ptrs,
                                                             _p(fic_ber), bptrs, _p(mer)), "dabgpu_decode_stream_frames_quality")
        return fib, ok, outs, fic_ber, msc_ber, mer

    def decode_stream_reset(self):
        _check(self._lib.dabgpu_decode_stream_reset(self._h), "dabgpu_decode_stream_reset")

    # ---- host arrays
    def ofdm_demod_frames(self, iq, freq_offset=None, want_cyc=False, want_dqpsk=False, soft=None):
        """iq: complex64 [n_frames][>=76*2552], row f starting at the first PRS sample."""
        iq = np.ascontiguousarray(iq, np.complex64)
        n_frames, stride = iq.shape
        if soft is None:
            soft = np.zeros((n_frames, NB_FRAME_BITS), np.int8)
        fo = None if freq_offset is None else np.ascontiguousarray(freq_offset, np.float32)
        cyc = np.zeros((n_frames, NB_SYMBOLS), np.complex64) if want_cyc else None
        dq = np.zeros((n_frames, NB_SYMBOLS - 1, NB_CARRIERS), np.complex64) if want_dqpsk else None
        _check(self._lib.dabgpu_ofdm_demod_frames(self._h, _p(iq), stride, n_frames, _p(fo), _p(soft), _p(cyc), _p(dq)),
               "dabgpu_ofdm_demod_frames")
        return soft, cyc, dq

    def fft_symbols(self, iq, freq_offset=None):
        iq = np.ascontiguousarray(iq, np.complex64)
        n_frames, stride = iq.shape
        fo = None if freq_offset is None else np.ascontiguousarray(freq_offset, np.float32)
        out = np.zeros((n_frames, NB_SYMBOLS, NB_FFT), np.complex64)
        _check(self._lib.dabgpu_fft_symbols(self._h, _p(iq), stride, n_frames, _p(fo), _p(out)), "dabgpu_fft_symbols")
        return out

    def sync_prs(self, iq, freq_offset=None, max_coarse=200):
        """iq: complex64 [n][>=2552], row f starting at the candidate first sample of the PRS cyclic prefix.
        -> structured array with coarse_carriers, time_offset, peak_to_mean, coarse_peak_to_mean."""
        iq = np.ascontiguousarray(iq, np.complex64)
        n, stride = iq.shape
        fo = None if freq_offset is None else np.ascontiguousarray(freq_offset, np.float32)
        out = np.zeros(n, dtype=[("coarse_carriers", np.int32), ("time_offset", np.int32),
                                 ("peak_to_mean", np.float32), ("coarse_peak_to_mean", np.float32)])
        _check(self._lib.dabgpu_sync_prs(self._h, _p(iq), stride, n, _p(fo), max_coarse, _p(out)), "dabgpu_sync_prs")
        return out

    def set_soft_selection(self, ranges):
        """ranges: iterable of (first_bit, count) in frame-bit coordinates, or None / empty for whole frames."""
        arr = np.array(list(ranges) if ranges is not None else [], np.int32).reshape(-1, 2)
        _check(self._lib.dabgpu_ofdm_set_soft_selection(self._h, _p(arr) if len(arr) else None, len(arr)),
               "dabgpu_ofdm_set_soft_selection")

    def acquire(self, iq, max_frames, cfg=None):
        """iq: complex64 [n_streams][n_samples] unaligned captures -> (frames [n_streams][max_frames] structured
        array (ACQUIRED_FRAME_DTYPE), counts [n_streams])."""
        iq = np.ascontiguousarray(iq, np.complex64)
        n_streams, n_samples = iq.shape
        out = np.zeros((n_streams, max_frames), ACQUIRED_FRAME_DTYPE)
        counts = np.zeros(n_streams, np.int32)
        _check(self._lib.dabgpu_acquire(self._h, _p(iq), n_samples, n_streams, n_samples,
                                    None if cfg is None else C.byref(cfg), max_frames, _p(out), _p(counts)), "dabgpu_acquire")
        return out, counts

    def acquire_dev(self, d_iq, stream_stride, n_streams, n_samples, max_frames, d_out, d_counts, cfg=None, stream=None):
        _check(self._lib.dabgpu_acquire_dev(self._h, d_iq, stream_stride, n_streams, n_samples,
                                        None if cfg is None else C.byref(cfg), max_frames, d_out, d_counts, stream),
               "dabgpu_acquire_dev")

    def ofdm_demod_acquired_dev(self, d_iq, stream_stride, n_streams, max_frames, d_frames, d_soft, d_cyc=None,
                                d_dqpsk=None, stream=None):
        _check(self._lib.dabgpu_ofdm_demod_acquired_dev(self._h, d_iq, stream_stride, n_streams, max_frames, d_frames, d_soft,
                                                    d_cyc, d_dqpsk, stream), "dabgpu_ofdm_demod_acquired_dev")

    def tii_frames_dev(self, d_iq, frame_stride, n_streams, frames_per_stream, d_acc, d_freq_offset=None, d_frame=None,
                       stream=None):
        """Transmitter identification of frames (s, f) at d_iq + (s*frames_per_stream + f)*frame_stride (PRS prefix; the 2656
        samples before are read): d_acc [n_streams] (TII_ACC_DTYPE) += the streams' frames; d_frame, if given, every frame's
        record.  d_freq_offset None = the stream states' fine + coarse offsets."""
        _check(self._lib.dabgpu_tii_frames_dev(self._h, d_iq, frame_stride, n_streams, frames_per_stream, d_freq_offset,
                                               d_frame, d_acc, stream), "dabgpu_tii_frames_dev")

    def tii_acquired_dev(self, d_iq, stream_stride, n_streams, max_frames, d_frames, d_acc, timing_margin=64, d_frame=None,
                         stream=None):
        """Transmitter identification of the locked, whole frames of acquire_dev / ofdm_demod_tracked_dev slots
        (PRS prefix at start + timing_margin) whose null window lies inside the capture."""
        _check(self._lib.dabgpu_tii_acquired_dev(self._h, d_iq, stream_stride, n_streams, max_frames, d_frames, timing_margin,
                                                 d_frame, d_acc, stream), "dabgpu_tii_acquired_dev")

    def cir_frames_dev(self, d_iq, frame_stride, n_streams, frames_per_stream, d_acc, d_freq_offset=None, d_frame=None,
                       stream=None):
        """Channel impulse response of frames (s, f) whose PRS prefix is at d_iq + (s*frames_per_stream + f)*frame_stride
        (the 2552 samples from it are read): d_acc [n_streams] (CIR_ACC_DTYPE) += the streams' frames; d_frame, if given,
        every frame's record.  d_freq_offset None = the stream states' fine + coarse offsets."""
        _check(self._lib.dabgpu_cir_frames_dev(self._h, d_iq, frame_stride, n_streams, frames_per_stream, d_freq_offset,
                                               d_frame, d_acc, stream), "dabgpu_cir_frames_dev")

    def cir_acquired_dev(self, d_iq, stream_stride, n_streams, max_frames, d_frames, d_acc, timing_margin=64, d_frame=None,
                         stream=None):
        """Channel impulse response of the locked, whole frames of acquire_dev / ofdm_demod_tracked_dev slots (PRS prefix
        at start + timing_margin, inside the capture)."""
        _check(self._lib.dabgpu_cir_acquired_dev(self._h, d_iq, stream_stride, n_streams, max_frames, d_frames, timing_margin,
                                                 d_frame, d_acc, stream), "dabgpu_cir_acquired_dev")

    def eti_frames_dev(self, plan, n_streams, frames_per_stream, d_fib, d_crc_ok, d_out, d_eti, d_status, d_history_in=None,
                       d_history_out=None, d_cif_start=None, stream=None):
        """ETI(NI) frames from what a decode call left on the device (dabgpu_eti_frames_dev): d_fib, d_crc_ok and d_out
        (list of device addresses in the order the plan's streams were given to eti_layout) -> d_eti [n_streams]
        [frames_per_stream*4][6144], d_status (ETI_STATUS_DTYPE); frame t carries the FIC of CIF t - 15, which the
        histories (ETI_HISTORY_DTYPE [n_streams]) carry from call to call.  Enqueues only."""
        n = plan.nst
        ptrs = (C.c_void_p * n)(*[C.c_void_p(x) for x in d_out]) if n else None
        if n and len(d_out) != n:
            raise ValueError("the plan has %d streams, d_out %d" % (n, len(d_out)))
        _check(self._lib.dabgpu_eti_frames_dev(self._h, C.byref(plan), n_streams, frames_per_stream, d_fib, d_crc_ok, ptrs,
                                               d_history_in, d_history_out, d_cif_start, d_eti, d_status, stream),
               "dabgpu_eti_frames_dev")

    def edi_frames_dev(self, plan, n_streams, frames_per_stream, d_fib, d_crc_ok, d_out, d_edi, stream_stride, d_status,
                       seq_start=None, d_history_in=None, d_history_out=None, d_cif_start=None, stream=None):
        """EDI from what a decode call left on the device (dabgpu_edi_frames_dev): the arguments of eti_frames_dev -> one AF
        packet per CIF, the 4 * frames_per_stream packets of stream s back to back from d_edi + s * stream_stride (both
        16-byte aligned), d_status (ETI_STATUS_DTYPE, length = edi_packet_bytes(plan)).  seq_start: the first packet's SEQ per
        stream (a sequence of n_streams numbers, None: 0).  Enqueues only."""
        n = plan.nst
        ptrs = (C.c_void_p * n)(*[C.c_void_p(x) for x in d_out]) if n else None
        if n and len(d_out) != n:
            raise ValueError("the plan has %d streams, d_out %d" % (n, len(d_out)))
        seq = None
        if seq_start is not None:
            if len(seq_start) != n_streams:
                raise ValueError("seq_start has %d entries for %d streams" % (len(seq_start), n_streams))
            seq = (C.c_uint32 * max(n_streams, 1))(*[int(x) & 0xFFFFFFFF for x in seq_start])
        _check(self._lib.dabgpu_edi_frames_dev(self._h, C.byref(plan), n_streams, frames_per_stream, d_fib, d_crc_ok, ptrs,
                                               d_history_in, d_history_out, d_cif_start, seq, d_edi, stream_stride, d_status,
                                               stream), "dabgpu_edi_frames_dev")

    def _decode_for_contribution(self, soft, n_streams, streams, history):
        """decode_frames_dev on device tensors, for decode_frames_eti / decode_frames_edi -> what their writer call takes"""
        import torch
        streams = [s if isinstance(s, EtiStream) else EtiStream(int(s[0]), s[1]) for s in streams]
        plan = eti_layout(streams)
        scs = [s.sc for s in streams]
        if soft.dtype != torch.int8 or soft.dim() != 2 or soft.stride(1) != 1 or soft.shape[0] % n_streams:
            raise ValueError("soft must be an int8 tensor [n_streams*frames_per_stream][>= 230400]")
        dev = soft.device
        n_frames = soft.shape[0]
        fps = n_frames // n_streams
        n_cif = fps * 4
        u8 = dict(dtype=torch.uint8, device=dev)
        fib = torch.empty((n_frames, 12, 32), **u8)
        ok = torch.empty((n_frames, 12), **u8)
        nbytes = [self._lib.dabgpu_subchannel_bytes(C.byref(sc)) for sc in scs]
        for nb in nbytes:
            _check(min(nb, 0), "dabgpu_subchannel_bytes")
        outs = [torch.empty((n_streams, n_cif, nb), **u8) for nb in nbytes]
        if history is None:
            msc_in, eti_in = None, None
        else:
            msc_in, eti_in = history
        msc_out = [torch.empty((n_streams, 15, sc.length * 64), dtype=torch.int8, device=dev) for sc in scs]
        eti_out = torch.empty((n_streams, eti_history_bytes()), **u8)
        status = torch.empty((n_streams, n_cif, 8), **u8)
        # the library's stream is not ordered behind torch's: what torch has enqueued for these tensors comes first
        torch.cuda.current_stream(dev).synchronize()
        self.decode_frames_dev(soft.data_ptr(), soft.stride(0), n_streams, fps, fib.data_ptr(), ok.data_ptr(), scs,
                               None if msc_in is None else [t.data_ptr() for t in msc_in], [t.data_ptr() for t in msc_out],
                               [t.data_ptr() for t in outs])
        return plan, fps, n_cif, fib, ok, outs, status, eti_in, (msc_out, eti_out)

    def decode_frames_eti(self, soft, n_streams, streams, history=None):
        """Soft bits (torch int8 tensor on this context's device, [n_streams*frames_per_stream][>= 230400]) -> ETI(NI):
        decode_frames_dev + eti_frames_dev on device tensors.  streams: [(subchannel_id, Subchannel), ...].
        history: what an earlier call on the same streams returned (None: the streams start here).
        -> (eti uint8 [n_streams, n_cif, 6144], status uint8 [n_streams, n_cif, 8] (view as ETI_STATUS_DTYPE on the host),
        history); all device tensors, the work is finished when the call returns."""
        import torch
        plan, fps, n_cif, fib, ok, outs, status, eti_in, hist = self._decode_for_contribution(soft, n_streams, streams, history)
        eti = torch.empty((n_streams, n_cif, ETI_FRAME_BYTES), dtype=torch.uint8, device=soft.device)
        self.eti_frames_dev(plan, n_streams, fps, fib.data_ptr(), ok.data_ptr(), [t.data_ptr() for t in outs], eti.data_ptr(),
                            status.data_ptr(), d_history_in=None if eti_in is None else eti_in.data_ptr(),
                            d_history_out=hist[1].data_ptr())
        self.sync()
        return eti, status, hist

    def decode_frames_edi(self, soft, n_streams, streams, history=None, seq_start=None):
        """decode_frames_eti with EDI out: decode_frames_dev + edi_frames_dev on device tensors.  seq_start: the first packet's
        SEQ per stream (None: 0); the caller adds n_cif per call.
        -> (edi uint8 [n_streams, n_cif * edi_packet_bytes(plan)], every stream's AF packets back to back, status uint8
        [n_streams, n_cif, 8] (ETI_STATUS_DTYPE), history -- the record of decode_frames_eti: either call continues the other)."""
        import torch
        plan, fps, n_cif, fib, ok, outs, status, eti_in, hist = self._decode_for_contribution(soft, n_streams, streams, history)
        stride = (n_cif * edi_packet_bytes(plan) + 15) // 16 * 16
        edi = torch.zeros((n_streams, stride), dtype=torch.uint8, device=soft.device)
        torch.cuda.current_stream(soft.device).synchronize()
        self.edi_frames_dev(plan, n_streams, fps, fib.data_ptr(), ok.data_ptr(), [t.data_ptr() for t in outs], edi.data_ptr(), stride,
                            status.data_ptr(), seq_start=seq_start, d_history_in=None if eti_in is None else eti_in.data_ptr(),
                            d_history_out=hist[1].data_ptr())
        self.sync()
        return edi[:, :n_cif * edi_packet_bytes(plan)], status, hist

    def modulate_eti_dev(self, plan, streams, n_streams, frames_per_stream, d_eti, d_iq, d_status, cfg=None, d_state_in=None,
                         d_state_out=None, frame_stride=NB_FRAME_SAMPLES, stream=None):
        """ETI(NI) frames d_eti [n_streams][frames_per_stream*4][6144] -> Mode-I IQ d_iq [n_streams*frames_per_stream] frames of
        complex64, frame_stride samples apart, and d_status (MOD_STATUS_DTYPE) per transmission frame
        (dabgpu_modulate_eti_dev).  streams: the list eti_layout made `plan` from.  The states (mod_state_bytes() per stream)
        carry the time interleaver from call to call.  Enqueues only."""
        items = [s if isinstance(s, EtiStream) else EtiStream(int(s[0]), s[1]) for s in streams]
        arr = (EtiStream * max(len(items), 1))(*items)
        if len(items) != plan.nst:
            raise ValueError("the plan has %d streams, the list %d" % (plan.nst, len(items)))
        _check(self._lib.dabgpu_modulate_eti_dev(self._h, C.byref(plan), arr, None if cfg is None else C.byref(cfg), n_streams,
                                                 frames_per_stream, d_eti, d_state_in, d_state_out, d_iq, frame_stride, d_status,
                                                 stream), "dabgpu_modulate_eti_dev")

    def modulate_eti(self, eti, streams, cfg=None, state=None, frame_stride=NB_FRAME_SAMPLES, out=None):
        """eti: torch uint8 tensor [n_streams][n_cif][6144] on this context's device (n_cif a multiple of 4); streams:
        [(subchannel_id, Subchannel) or EtiStream, ...] (eti_streams(frame) reads them from a frame).  state: what an earlier
        call on the same streams returned (None: the streams start here).  out: a complex64 tensor
        [n_streams * n_cif / 4][frame_stride] to write into (only the 196 608 samples of every frame are touched).
        -> (iq complex64 [n_frames][frame_stride], status uint8 [n_frames][8] (view as MOD_STATUS_DTYPE on the host), state);
        device tensors, the work is finished when the call returns."""
        import torch
        if eti.dtype != torch.uint8 or eti.dim() != 3 or eti.shape[2] != ETI_FRAME_BYTES or eti.shape[1] % 4 or not eti.is_contiguous():
            raise ValueError("eti must be a contiguous uint8 tensor [n_streams][4 * frames][6144]")
        items = [s if isinstance(s, EtiStream) else EtiStream(int(s[0]), s[1]) for s in streams]
        plan = eti_layout(items)
        dev = eti.device
        n_streams, fps = eti.shape[0], eti.shape[1] // 4
        n_frames = n_streams * fps
        if out is None:
            out = torch.empty((n_frames, frame_stride), dtype=torch.complex64, device=dev)
        elif out.dtype != torch.complex64 or tuple(out.shape) != (n_frames, frame_stride) or not out.is_contiguous():
            raise ValueError("out must be a contiguous complex64 tensor [%d][%d]" % (n_frames, frame_stride))
        status = torch.empty((n_frames, 8), dtype=torch.uint8, device=dev)
        state_out = torch.empty((n_streams, mod_state_bytes()), dtype=torch.uint8, device=dev)
        # the library's stream is not ordered behind torch's: what torch has enqueued for these tensors comes first
        torch.cuda.current_stream(dev).synchronize()
        self.modulate_eti_dev(plan, items, n_streams, fps, eti.data_ptr(), out.data_ptr(), status.data_ptr(), cfg=cfg,
                              d_state_in=None if state is None else state.data_ptr(), d_state_out=state_out.data_ptr(),
                              frame_stride=frame_stride)
        self.sync()
        return out, status, state_out

    def eti_read_dev(self, entries, stream=None):
        """ETI(NI) byte streams -> FIBs, CRC flags and logical frames on the device (dabgpu_eti_read_dev): entries is a list
        of EtiReadEntry (device addresses), each a stream with its own plan, byte count and state.  Enqueues only."""
        _entries_call("dabgpu_eti_read_dev", EtiReadEntry, entries, stream, ctx=self)

    def edi_read_dev(self, entries, stream=None):
        """AF packet byte streams -> FIBs, CRC flags and logical frames on the device (dabgpu_edi_read_dev): entries is a list
        of EdiReadEntry (device addresses), each a stream with its own plan, byte count and state.  Enqueues only."""
        _entries_call("dabgpu_edi_read_dev", EtiReadEntry, entries, stream, ctx=self)

    def edi_read(self, bytes_tensor, streams, state=None):
        """bytes_tensor: torch uint8 tensor [n_streams][n_bytes] on this context's device, the next n_bytes of n_streams AF
        packet byte streams of ONE multiplex (n_bytes a multiple of 16 unless there is one stream, so that every row is
        aligned); streams: [(subchannel_id, Subchannel) or EtiStream, ...], or None for the discovery pass (only the FIC
        leaves).  state: what an earlier call on the same streams returned (None: the streams start here).
        -> (fib uint8 [n_streams][max_rows][3][32], crc_ok uint8 [n_streams][max_rows][3], outs: one uint8 tensor [n_streams]
        [max_rows][bitrate * 3] per stream in the order of `streams`, status uint8 [n_streams][max_rows][32] (view as
        EDI_READ_STATUS_DTYPE on the host), result uint8 [n_streams][48] (EDI_READ_RESULT_DTYPE), state); device tensors, zero
        behind a stream's emitted rows; the work is finished when the call returns."""
        import torch
        if bytes_tensor.dtype != torch.uint8 or bytes_tensor.dim() != 2 or not bytes_tensor.is_contiguous() or \
                (bytes_tensor.shape[0] > 1 and bytes_tensor.shape[1] % 16) or bytes_tensor.data_ptr() % 16:
            raise ValueError("bytes_tensor must be a contiguous, 16-byte aligned uint8 tensor [n_streams][n_bytes], n_bytes a multiple of 16 "
                             "unless there is one stream")
        plan, items = None, []
        if streams is not None:
            items = [s if isinstance(s, EtiStream) else EtiStream(int(s[0]), s[1]) for s in streams]
            plan = eti_layout(items)
        dev = bytes_tensor.device
        n_streams, n_bytes = bytes_tensor.shape
        rows = edi_read_max_rows(n_bytes, plan)
        u8 = dict(dtype=torch.uint8, device=dev)
        fib = torch.zeros((n_streams, rows, 3, 32), **u8)
        ok = torch.zeros((n_streams, rows, 3), **u8)
        outs = [torch.zeros((n_streams, rows, s.sc.bitrate_kbps * 3), **u8) for s in items]
        status = torch.zeros((n_streams, rows, 32), **u8)
        result = torch.zeros((n_streams, 48), **u8)
        state_out = torch.empty((n_streams, edi_read_state_bytes()), **u8)
        entries, keep = [], []
        for s in range(n_streams):
            ptrs = (C.c_void_p * max(len(items), 1))(*[o[s].data_ptr() for o in outs])
            keep.append(ptrs)
            entries.append(EdiReadEntry(bytes_tensor[s].data_ptr() if n_bytes else None, n_bytes, 0,
                                        C.pointer(plan) if plan is not None else None,
                                        C.cast(ptrs, C.POINTER(C.c_void_p)) if plan is not None else None,
                                        None if state is None else state[s].data_ptr(), state_out[s].data_ptr(),
                                        fib[s].data_ptr(), ok[s].data_ptr(), status[s].data_ptr(), result[s].data_ptr()))
        # the library's stream is not ordered behind torch's: what torch has enqueued for these tensors comes first
        torch.cuda.current_stream(dev).synchronize()
        self.edi_read_dev(entries)
        self.sync()
        return fib, ok, outs, status, result, state_out

    def pft_fragments_dev(self, layout, n_streams, n_packets, d_af, in_stride, d_pf, out_stride, pseq_start=None, source=0, dest=0,
                          stream=None):
        """AF packets -> PF fragments on the device (dabgpu_pft_fragments_dev): n_packets packets of layout.packet_bytes back
        to back per stream from d_af + s * in_stride (what edi_frames_dev leaves) -> layout.stream_bytes per packet, back to
        back per stream from d_pf + s * out_stride (all 16-byte aligned).  pseq_start: the first packet's Pseq per stream, a
        HOST sequence (None: 0); the caller adds n_packets to it.  Enqueues only."""
        seq = None if pseq_start is None else (C.c_uint32 * max(n_streams, 1))(*[int(v) & 0xFFFFFFFF for v in pseq_start])
        _check(self._lib.dabgpu_pft_fragments_dev(self._h, C.byref(layout), n_streams, n_packets, d_af, in_stride, seq, int(source),
                                                  int(dest), d_pf, out_stride, stream), "dabgpu_pft_fragments_dev")

    def pft_fragments(self, layout, af, pseq_start=None, source=0, dest=0):
        """pft_fragments_dev on a torch uint8 tensor [n_streams][n_packets * layout.packet_bytes] (row stride a multiple of 16
        unless there is one stream) -> uint8 tensor [n_streams][n_packets * layout.stream_bytes]; finished on return."""
        import torch
        n_streams, n_in = af.shape
        n_packets = n_in // layout.packet_bytes
        if af.dtype != torch.uint8 or n_packets * layout.packet_bytes != n_in or af.stride(1) != 1 or af.data_ptr() % 16 or \
                (n_streams > 1 and af.stride(0) % 16):
            raise ValueError("af must be a 16-byte aligned uint8 tensor of whole packets, its row stride a multiple of 16")
        out_stride = (n_packets * layout.stream_bytes + 15) // 16 * 16
        out = torch.zeros((n_streams, out_stride), dtype=torch.uint8, device=af.device)
        in_stride = af.stride(0) if n_streams > 1 else (n_in + 15) // 16 * 16
        torch.cuda.current_stream(af.device).synchronize()
        self.pft_fragments_dev(layout, n_streams, n_packets, af.data_ptr(), in_stride, out.data_ptr(), out_stride, pseq_start, source, dest)
        self.sync()
        return out[:, :n_packets * layout.stream_bytes]

    def pft_read_dev(self, entries, stream=None):
        """PF fragment byte streams -> AF packet byte streams on the device (dabgpu_pft_read_dev): entries is a list of
        PftReadEntry (device addresses), each a stream with its own byte count, flags and state.  Enqueues only."""
        _entries_call("dabgpu_pft_read_dev", PftReadEntry, entries, stream, ctx=self)

    def pft_read(self, bytes_tensor, state=None, flush=False):
        """bytes_tensor: torch uint8 tensor [n_streams][n_bytes] on this context's device, the next n_bytes of n_streams PF
        fragment byte streams (n_bytes a multiple of 16 unless there is one stream).  state: what an earlier call on the same
        streams returned (None: the streams start here); flush: close every open group at the end.
        -> (out uint8 [n_streams][pft_read_out_bytes(n_bytes)], the AF packets of stream s back to back in its first
        result["out_bytes"] bytes; records uint8 [n_streams][max_records][32] (view as PFT_READ_RECORD_DTYPE on the host),
        result uint8 [n_streams][64] (PFT_READ_RESULT_DTYPE), state); device tensors; the work is finished when the call
        returns.  To hand a stream on to edi_read its out_bytes has to come to the host first."""
        import torch
        if bytes_tensor.dtype != torch.uint8 or bytes_tensor.dim() != 2 or not bytes_tensor.is_contiguous() or \
                (bytes_tensor.shape[0] > 1 and bytes_tensor.shape[1] % 16) or bytes_tensor.data_ptr() % 16:
            raise ValueError("bytes_tensor must be a contiguous, 16-byte aligned uint8 tensor [n_streams][n_bytes], n_bytes a multiple of 16 "
                             "unless there is one stream")
        dev = bytes_tensor.device
        n_streams, n_bytes = bytes_tensor.shape
        u8 = dict(dtype=torch.uint8, device=dev)
        out = torch.zeros((n_streams, pft_read_out_bytes(n_bytes)), **u8)
        records = torch.zeros((n_streams, pft_read_max_records(n_bytes), 32), **u8)
        result = torch.zeros((n_streams, 64), **u8)
        state_out = torch.empty((n_streams, pft_read_state_bytes()), **u8)
        entries = [PftReadEntry(bytes_tensor[s].data_ptr() if n_bytes else None, n_bytes, PFT_READ_FLUSH if flush else 0,
                                None if state is None else state[s].data_ptr(), state_out[s].data_ptr(), out[s].data_ptr(),
                                records[s].data_ptr(), result[s].data_ptr()) for s in range(n_streams)]
        # the library's stream is not ordered behind torch's: what torch has enqueued for these tensors comes first
        torch.cuda.current_stream(dev).synchronize()
        self.pft_read_dev(entries)
        self.sync()
        return out, records, result, state_out

    def eti_read(self, bytes_tensor, streams, state=None):
        """bytes_tensor: torch uint8 tensor [n_streams][n_bytes] on this context's device, the next n_bytes of n_streams ETI(NI)
        byte streams of ONE multiplex (n_bytes a multiple of 16 unless there is one stream, so that every row is aligned); streams: [(subchannel_id,
        Subchannel) or EtiStream, ...], or None for the discovery pass (only the FIC leaves).  state: what an earlier call on
        the same streams returned (None: the streams start here).
        -> (fib uint8 [n_streams][max_frames][3][32], crc_ok uint8 [n_streams][max_frames][3], outs: one uint8 tensor
        [n_streams][max_frames][bitrate * 3] per stream in the order of `streams`, status uint8 [n_streams][max_frames][16]
        (view as ETI_READ_STATUS_DTYPE on the host), result uint8 [n_streams][48] (ETI_READ_RESULT_DTYPE), state); device
        tensors, zero behind a stream's emitted rows; the work is finished when the call returns."""
        import torch
        if bytes_tensor.dtype != torch.uint8 or bytes_tensor.dim() != 2 or not bytes_tensor.is_contiguous() or \
                (bytes_tensor.shape[0] > 1 and bytes_tensor.shape[1] % 16) or bytes_tensor.data_ptr() % 16:
            raise ValueError("bytes_tensor must be a contiguous, 16-byte aligned uint8 tensor [n_streams][n_bytes], n_bytes a multiple of 16 "
                             "unless there is one stream")
        plan, items = None, []
        if streams is not None:
            items = [s if isinstance(s, EtiStream) else EtiStream(int(s[0]), s[1]) for s in streams]
            plan = eti_layout(items)
        dev = bytes_tensor.device
        n_streams, n_bytes = bytes_tensor.shape
        rows = eti_read_max_frames(n_bytes)
        u8 = dict(dtype=torch.uint8, device=dev)
        fib = torch.zeros((n_streams, rows, 3, 32), **u8)
        ok = torch.zeros((n_streams, rows, 3), **u8)
        outs = [torch.zeros((n_streams, rows, s.sc.bitrate_kbps * 3), **u8) for s in items]
        status = torch.zeros((n_streams, rows, 16), **u8)
        result = torch.zeros((n_streams, 48), **u8)
        state_out = torch.empty((n_streams, eti_read_state_bytes()), **u8)
        entries, keep = [], []
        for s in range(n_streams):
            ptrs = (C.c_void_p * max(len(items), 1))(*[o[s].data_ptr() if rows else 0 for o in outs])
            keep.append(ptrs)
            entries.append(EtiReadEntry(bytes_tensor[s].data_ptr() if n_bytes else None, n_bytes, 0,
                                        C.pointer(plan) if plan is not None else None,
                                        C.cast(ptrs, C.POINTER(C.c_void_p)) if plan is not None else None,
                                        None if state is None else state[s].data_ptr(), state_out[s].data_ptr(),
                                        fib[s].data_ptr() if rows else None, ok[s].data_ptr() if rows else None,
                                        status[s].data_ptr() if rows else None, result[s].data_ptr()))
        # the library's stream is not ordered behind torch's: what torch has enqueued for these tensors comes first
        torch.cuda.current_stream(dev).synchronize()
        self.eti_read_dev(entries)
        self.sync()
        return fib, ok, outs, status, result, state_out

    def dabplus_superframes(self, sfs, bitrate_kbps, out=None, status=None):
        """sfs: uint8 [n][>=15*bitrate] aligned super-frames -> (data [n][110*s], status [n] SUPERFRAME_STATUS_DTYPE).
        out / status: the caller's own arrays of those shapes (page-locked ones take the library's page-locked path)."""
        sfs = np.ascontiguousarray(sfs, np.uint8)
        n, stride = sfs.shape
        s = bitrate_kbps // 8
        if out is None:
            out = np.zeros((n, 110 * s), np.uint8)
        if status is None:
            status = np.zeros(n, SUPERFRAME_STATUS_DTYPE)
        if out.dtype != np.uint8 or out.shape != (n, 110 * s) or not out.flags.c_contiguous:
            raise ValueError("out must be contiguous uint8 [%d][%d]" % (n, 110 * s))
        if status.dtype != SUPERFRAME_STATUS_DTYPE or status.shape != (n,) or not status.flags.c_contiguous:
            raise ValueError("status must be contiguous SUPERFRAME_STATUS_DTYPE [%d]" % n)
        _check(self._lib.dabgpu_dabplus_superframes(self._h, _p(sfs), stride, n, bitrate_kbps, _p(out), _p(status)),
               "dabgpu_dabplus_superframes")
        return out, status

    def dabplus_superframes_dev(self, d_in, in_stride, n, bitrate_kbps, d_out, d_status, stream=None):
        """Device pointers: super-frame f at d_in + f * in_stride (120*s bytes) -> d_out [n][110*s], d_status [n]
        (SUPERFRAME_STATUS_DTYPE)."""
        _check(self._lib.dabgpu_dabplus_superframes_dev(self._h, d_in, in_stride, n, bitrate_kbps, d_out, d_status, stream),
               "dabgpu_dabplus_superframes_dev")

    def dabplus_follow_dev(self, entries, n_cifs, stream=None):
        """Follow DAB+ sub-channels to super-frames on the device: entries is a list of DabplusEntry (device addresses; any
        mix of bit rates), each with n_cifs new logical frames.  Per entry: d_data / d_status rows [0, n_superframes),
        d_result (DABPLUS_FOLLOW_RESULT_DTYPE) and d_carry_out, to be passed as d_carry_in of the next call."""
        _entries_call("dabgpu_dabplus_follow_dev", DabplusEntry, entries, n_cifs, stream, ctx=self)

    def mp2_follow_dev(self, entries, n_cifs, stream=None):
        """Follows DAB (MPEG layer II) sub-channels to checked frames and PAD rows on the device: entries is a list of Mp2Entry
        (device addresses), n_cifs the logical frames every entry's d_in holds.  Per entry: d_rows [n_cifs + 1][MP2_ROW_BYTES],
        d_status (SUPERFRAME_STATUS_DTYPE), d_follow (DABPLUS_FOLLOW_RESULT_DTYPE: what PadEntry / MotEntry.d_follow point at,
        with bitrate_kbps = MP2_PAD_KBPS), d_result (MP2_RESULT_DTYPE).  No host synchronisation."""
        _entries_call("dabgpu_mp2_follow_dev", Mp2Entry, entries, n_cifs, stream, ctx=self)

    def mp2_subbands_dev(self, entries, n_cifs, stream=None):
        """Behind mp2_follow_dev on the same stream: decodes every checked frame of every entry (a list of Mp2AudioEntry, device
        addresses, n_cifs as in the follow call) to sub-band samples -- everything of layer II but the synthesis filter.  Per
        entry: d_levels [n_cifs + 1] (MP2_LEVEL_DTYPE; rows at or beyond the follow call's `frames` are not written),
        d_subbands NULL or [n_cifs + 1] + MP2_SUBBANDS_SHAPE float32, d_audio (MP2_AUDIO_RESULT_DTYPE).  No host
        synchronisation."""
        _entries_call("dabgpu_mp2_subbands_dev", Mp2AudioEntry, entries, n_cifs, stream, ctx=self)

    def pad_labels_dev(self, entries, stream=None):
        """Dynamic labels of followed DAB+ sub-channels, behind dabplus_follow_dev on the same stream: entries is a list of
        PadEntry (device addresses).  Per entry: d_label (PAD_LABEL_DTYPE), d_result (PAD_RESULT_DTYPE, counts of this call)
        and d_state_out, to be passed as d_state_in of the next call."""
        _entries_call("dabgpu_pad_labels_dev", PadEntry, entries, stream, ctx=self)

    def mot_slides_dev(self, entries, stream=None):
        """Slideshow objects of followed DAB+ sub-channels, behind dabplus_follow_dev on the same stream: entries is a list
        of MotEntry (device addresses).  Per entry: completed objects in the slots of d_slides (MOT_SLIDE_DTYPE, the MOT
        header, the body), d_result (MOT_RESULT_DTYPE, counts of this call), d_state_out, to be passed as d_state_in of the
        next call, and d_arena, which goes into the next call as it is."""
        _entries_call("dabgpu_mot_slides_dev", MotEntry, entries, stream, ctx=self)

    def packet_slides_dev(self, entries, n_cifs, stream=None):
        """Slideshow objects of packet-mode MOT components, behind decode_ensembles_dev on the same stream: entries is a list
        of PacketEntry (device addresses), one per (sub-channel, packet address); n_cifs logical frames each.  Per entry:
        completed objects in the slots of d_slides (MOT_SLIDE_DTYPE, the MOT header, the body), d_result
        (PACKET_RESULT_DTYPE, counts of this call), d_state_out, to be passed as d_state_in of the next call, and d_arena,
        which goes into the next call as it is.  No host synchronisation."""
        _entries_call("dabgpu_packet_slides_dev", PacketEntry, entries, n_cifs, stream, ctx=self)

    def packet_carousel_dev(self, entries, n_cifs, stream=None):
        """Objects of packet-mode MOT directory carousels, behind decode_ensembles_dev (and either FEC call) on the same
        stream: entries is a list of PacketCarouselEntry (device addresses), one per (sub-channel, packet address); n_cifs
        logical frames each.  Per entry: d_objects slots of a MOT_CAROUSEL_OBJECT_DTYPE record, the MOT header from the
        directory and the body; d_directory, the current directory's bytes; d_result, a PACKET_CAROUSEL_RESULT_DTYPE record.
        No host synchronisation."""
        _entries_call("dabgpu_packet_carousel_dev", PacketCarouselEntry, entries, n_cifs, stream, ctx=self)

    def packet_groups_dev(self, entries, n_cifs, stream=None):
        """The MSC data groups (mode 0) or the raw useful bytes (mode 1) of any packet-mode component, behind
        decode_ensembles_dev (and either FEC call) on the same stream: entries is a list of PacketGroupsEntry (device
        addresses), one per (sub-channel, packet address); n_cifs logical frames each.  Per entry: the groups' bytes in
        d_bytes, a DATA_GROUP_DTYPE record each in d_groups, d_result (PACKET_GROUPS_RESULT_DTYPE, counts of this call) and
        d_state_out, to be passed as d_state_in of the next call.  No host synchronisation."""
        _entries_call("dabgpu_packet_groups_dev", PacketGroupsEntry, entries, n_cifs, stream, ctx=self)

    def dmb_follow_dev(self, entries, n_cifs, stream=None):
        """T-DMB stream-mode sub-channels to checked TS packets on the device (dabgpu_dmb_follow_dev): entries is a list of
        DmbEntry (device addresses), one per (stream, sub-channel), n_cifs logical frames each.  Per entry: d_ts, the
        emitted 188-byte packets back to back; d_records (DMB_RECORD_DTYPE); d_result (DMB_RESULT_DTYPE, counts of this
        call); d_state_out, which the next call takes as d_state_in.  Three launches whatever the number of entries, no
        host synchronisation."""
        _entries_call("dabgpu_dmb_follow_dev", DmbEntry, entries, n_cifs, stream, ctx=self)

    def dmb_follow(self, frames, bitrate, state=None):
        """frames: torch uint8 tensor [n_streams][n_cifs][row] on this context's device, row >= 3 * bitrate, the last dimension
        contiguous: the next logical frames of n_streams T-DMB sub-channels of one bit rate (what the decode call or the ETI /
        EDI readers wrote).  state: what an earlier call on the same streams returned (None: the streams start here).
        -> (ts uint8 [n_streams][max_packets][188], records uint8 [n_streams][max_packets][16] (view as DMB_RECORD_DTYPE on
        the host), result uint8 [n_streams][80] (DMB_RESULT_DTYPE; packets_emitted says how many of ts are packets), state
        uint8 [n_streams][dmb_state_bytes()]); device tensors; the work is finished when the call returns."""
        import torch
        if frames.dtype != torch.uint8 or frames.dim() != 3 or frames.shape[2] < 3 * bitrate or (frames.numel() and frames.stride(2) != 1):
            raise ValueError("frames must be a uint8 tensor [n_streams][n_cifs][>= 3 * bitrate] with contiguous rows")
        n_streams, n_cifs = frames.shape[0], frames.shape[1]
        m = dmb_max_packets(bitrate, n_cifs)
        u8 = dict(dtype=torch.uint8, device=frames.device)
        ts = torch.zeros((n_streams, (max(m, 1) * DMB_TS_BYTES + 15) // 16 * 16), **u8)    # (every stream's packets on a 16-byte boundary)
        records = torch.zeros((n_streams, max(m, 1), 16), **u8)
        result = torch.zeros((n_streams, 80), **u8)
        state_out = torch.empty((n_streams, dmb_state_bytes()), **u8)
        if n_cifs > 1 and n_streams and frames.stride(1) < 3 * bitrate:
            raise ValueError("rows overlap")
        entries = [DmbEntry(frames[s].data_ptr() if n_cifs else None, frames.stride(1) if n_cifs > 1 else max(frames.shape[2], 3 * bitrate),
                            bitrate, m, ts[s].data_ptr(), records[s].data_ptr(), None if state is None else state[s].data_ptr(),
                            state_out[s].data_ptr(), result[s].data_ptr()) for s in range(n_streams)]
        torch.cuda.current_stream(frames.device).synchronize()
        self.dmb_follow_dev(entries, n_cifs)
        self.sync()
        return ts[:, :m * DMB_TS_BYTES].unflatten(1, (m, DMB_TS_BYTES)), records[:, :m], result, state_out

    def packet_fec_dev(self, entries, n_cifs, stream=None):
        """RS(204,188) correction of the FEC frames of packet-mode sub-channels, between decode_ensembles_dev and
        packet_slides_dev on the same stream: entries is a list of PacketFecEntry (device addresses), one per sub-channel;
        n_cifs logical frames each.  Per entry: d_out, the stream delayed by packet_fec_delay(bitrate) frames and corrected
        (the slides call names it as d_in and keeps fec non-zero), d_result (PACKET_FEC_RESULT_DTYPE, counts of this call)
        and d_state_out, to be passed as d_state_in of the next call.  No host synchronisation."""
        _entries_call("dabgpu_packet_fec_dev", PacketFecEntry, entries, n_cifs, stream, ctx=self)

    def packet_fec_erasures_dev(self, entries, n_cifs, stream=None):
        """packet_fec_dev with the failed packet CRCs of the arriving frames as erasures (up to eight lost packets per FEC
        frame instead of four): entries is a list of PacketFecErasureEntry (device addresses); d_result is a
        PACKET_FEC_ERASURE_RESULT_DTYPE record.  What packet_fec_dev corrects, this call corrects identically; its state
        record is its own (one of packet_fec_dev is a fresh start).  No host synchronisation."""
        _entries_call("dabgpu_packet_fec_erasures_dev", PacketFecErasureEntry, entries, n_cifs, stream, ctx=self)

    def fic_decode(self, soft):
        """soft: int8 [n_frames][>=9216]."""
        soft = np.ascontiguousarray(soft, np.int8)
        n_frames, stride = soft.shape
        fib = np.zeros((n_frames, 12, 32), np.uint8)
        ok = np.zeros((n_frames, 12), np.uint8)
        _check(self._lib.dabgpu_fic_decode(self._h, _p(soft), stride, n_frames, _p(fib), _p(ok)), "dabgpu_fic_decode")
        return fib, ok

    def msc_decode(self, sc, soft, n_streams, history_in=None, want_history=False):
        """soft: int8 [n_streams*frames_per_stream][230400]."""
        soft = np.ascontiguousarray(soft, np.int8)
        n_frames, stride = soft.shape
        fps = n_frames // n_streams
        nbytes = self._lib.dabgpu_subchannel_bytes(C.byref(sc))
        _check(min(nbytes, 0), "dabgpu_subchannel_bytes")
        out = np.zeros((n_streams, fps * 4, nbytes), np.uint8)
        hi = None if history_in is None else np.ascontiguousarray(history_in, np.int8)
        ho = np.zeros((n_streams, 15, sc.length * 64), np.int8) if want_history else None
        _check(self._lib.dabgpu_msc_decode(self._h, C.byref(sc), _p(soft), stride, n_streams, fps, _p(hi), _p(ho), _p(out)),
               "dabgpu_msc_decode")
        return out, ho

    def viterbi(self, punct, mask):
        """punct: int8 [n_codewords][n_punct]; mask: uint8 [4*nsteps] -> bytes [n][(nsteps-6)/8]."""
        punct = np.ascontiguousarray(punct, np.int8)
        mask = np.ascontiguousarray(mask, np.uint8)
        nsteps = mask.size // 4
        n = punct.shape[0]
        out = np.zeros((n, (nsteps - 6) // 8), np.uint8)
        _check(self._lib.dabgpu_viterbi(self._h, _p(punct), n, _p(mask), nsteps, _p(out)), "dabgpu_viterbi")
        return out

    # ---- device pointers (ints), enqueue only
    def ofdm_demod_frames_dev(self, d_iq, frame_stride, n_frames, d_freq_offset, d_soft, d_cyc=None, d_dqpsk=None,
                              stream=None):
        _check(self._lib.dabgpu_ofdm_demod_frames_dev(self._h, d_iq, frame_stride, n_frames, d_freq_offset, d_soft,
                                                  d_cyc, d_dqpsk, stream), "dabgpu_ofdm_demod_frames_dev")

    def ofdm_demod_frames_dd_dev(self, d_iq, frame_stride, n_frames, d_freq_offset, d_soft, d_dd4, stream=None):
        _check(self._lib.dabgpu_ofdm_demod_frames_dd_dev(self._h, d_iq, frame_stride, n_frames, d_freq_offset, d_soft, d_dd4,
                                                     stream), "dabgpu_ofdm_demod_frames_dd_dev")

    def sync_prs_dev(self, d_iq, frame_stride, n_frames, d_freq_offset, max_coarse, d_out, stream=None):
        """d_out: [n_frames] dabgpu_sync_result (4 x 32 bit: coarse_carriers, time_offset, peak_to_mean, coarse ptm)."""
        _check(self._lib.dabgpu_sync_prs_dev(self._h, d_iq, frame_stride, n_frames, d_freq_offset, max_coarse, d_out, stream),
               "dabgpu_sync_prs_dev")

    def fft_symbols_dev(self, d_iq, frame_stride, n_frames, d_freq_offset, d_spectra, stream=None):
        _check(self._lib.dabgpu_fft_symbols_dev(self._h, d_iq, frame_stride, n_frames, d_freq_offset, d_spectra, stream),
               "dabgpu_fft_symbols_dev")

    def fic_decode_dev(self, d_soft, soft_stride, n_frames, d_fib, d_crc_ok, stream=None):
        _check(self._lib.dabgpu_fic_decode_dev(self._h, d_soft, soft_stride, n_frames, d_fib, d_crc_ok, stream),
               "dabgpu_fic_decode_dev")

    def msc_decode_multi_dev(self, scs, d_soft, soft_stride, n_streams, frames_per_stream, d_hist_in, d_hist_out, d_out,
                             stream=None):
        """scs: list of Subchannel; d_hist_in/out, d_out: lists of device addresses (or None)."""
        n = len(scs)
        arr = (Subchannel * n)(*scs)
        def ptrs(lst):
            if lst is None:
                return None
            return (C.c_void_p * n)(*[C.c_void_p(x) if x else None for x in lst])
        hi, ho, out = ptrs(d_hist_in), ptrs(d_hist_out), ptrs(d_out)
        _check(self._lib.dabgpu_msc_decode_multi_dev(self._h, arr, n, d_soft, soft_stride, n_streams, frames_per_stream,
                                                 hi, ho, out, stream), "dabgpu_msc_decode_multi_dev")

    def decode_frames_dev(self, d_soft, soft_stride, n_streams, frames_per_stream, d_fib, d_crc_ok, scs, d_hist_in, d_hist_out,
                          d_out, stream=None):
        """FIC + the sub-channels `scs` of every frame in one call (lists of device addresses as msc_decode_multi_dev)."""
        n = len(scs)
        arr = (Subchannel * max(n, 1))(*scs)
        def ptrs(lst):
            if lst is None or n == 0:
                return None
            return (C.c_void_p * n)(*[C.c_void_p(x) if x else None for x in lst])
        _check(self._lib.dabgpu_decode_frames_dev(self._h, d_soft, soft_stride, n_streams, frames_per_stream, d_fib, d_crc_ok,
                                              arr, n, ptrs(d_hist_in), ptrs(d_hist_out), ptrs(d_out), stream),
               "dabgpu_decode_frames_dev")

    def decode_ensembles_dev(self, d_soft, soft_stride, n_streams, frames_per_stream, d_fib, d_crc_ok, scs, d_hist_in, d_hist_out,
                             d_out, stream=None, sc_first=None):
        """decode_frames_dev for ensembles that each have their own multiplex: scs, d_hist_in, d_hist_out, d_out are lists
        (one per stream) of lists (one per sub-channel of that stream) of Subchannel / device addresses; d_hist_in and
        d_hist_out may be None, d_fib and d_crc_ok both None (sub-channels only).  sc_first: the [n_streams + 1] offsets to
        pass instead of the ones the lists imply (the library checks them)."""
        if len(scs) != n_streams:
            raise ValueError("one sub-channel list per stream")
        flat = [sc for lst in scs for sc in lst]
        n = len(flat)
        if sc_first is None:
            sc_first = np.cumsum([0] + [len(lst) for lst in scs]).tolist()
        if len(sc_first) != n_streams + 1:
            raise ValueError("sc_first has n_streams + 1 entries")
        first = (C.c_int32 * (n_streams + 1))(*[int(x) for x in sc_first])
        arr = (Subchannel * max(n, 1))(*flat)
        def ptrs(lsts):
            if lsts is None or n == 0:
                return None
            vals = [x for lst in lsts for x in lst]
            if len(vals) != n:
                raise ValueError("one address per sub-channel of every stream")
            return (C.c_void_p * n)(*[C.c_void_p(x) if x else None for x in vals])
        _check(self._lib.dabgpu_decode_ensembles_dev(self._h, d_soft, soft_stride, n_streams, frames_per_stream, d_fib, d_crc_ok,
                                                     arr, first, ptrs(d_hist_in), ptrs(d_hist_out), ptrs(d_out), stream),
               "dabgpu_decode_ensembles_dev")

    def mer_dev(self, d_soft, soft_stride, n_frames, d_out, first_symbol=0, n_symbols=75, stream=None):
        """MER sums of data symbols [first_symbol, first_symbol + n_symbols) per frame -> d_out [n_frames] (MER_DTYPE)."""
        _check(self._lib.dabgpu_mer_dev(self._h, d_soft, soft_stride, n_frames, first_symbol, n_symbols, d_out, stream),
               "dabgpu_mer_dev")

    def channel_ber_dev(self, d_soft, soft_stride, n_streams, frames_per_stream, d_fib, d_fic, scs=(), d_hist_in=None, d_out=None,
                        d_msc=None, stream=None):
        """Channel BER counts (BER_DTYPE) of a decode enqueued before: d_fib / d_fic [n_frames][4] for the FIC (None: not
        counted), per sub-channel d_out[i] (decoded bytes) -> d_msc[i] [n_streams][frames_per_stream*4]; d_hist_in as the
        decode had it (lists of device addresses as msc_decode_multi_dev)."""
        n = len(scs)
        arr = (Subchannel * max(n, 1))(*scs)
        def ptrs(lst):
            if lst is None or n == 0:
                return None
            return (C.c_void_p * n)(*[C.c_void_p(x) if x else None for x in lst])
        _check(self._lib.dabgpu_channel_ber_dev(self._h, d_soft, soft_stride, n_streams, frames_per_stream, d_fib, d_fic, arr, n,
                                                ptrs(d_hist_in), ptrs(d_out), ptrs(d_msc), stream), "dabgpu_channel_ber_dev")

    def msc_decode_dev(self, sc, d_soft, soft_stride, n_streams, frames_per_stream, d_hist_in, d_hist_out, d_out,
                       stream=None):
        _check(self._lib.dabgpu_msc_decode_dev(self._h, C.byref(sc), d_soft, soft_stride, n_streams, frames_per_stream,
                                           d_hist_in, d_hist_out, d_out, stream), "dabgpu_msc_decode_dev")
