"""CPU-only checks of the C API's entry prologues: what every handle-taking entry point returns for a NULL handle, an unloaded
handle and arguments outside what it accepts, and in which order those checks run where several fail at once.  Only calls that
return before the first HIP call are made, so this runs on a machine without a GPU."""
import ctypes as C

import pytest

import rust_msbwt_amd as msbwt

_lib = msbwt._lib
OK, INVALID, NOT_LOADED = _lib.OK, _lib.ERR_INVALID_ARG, _lib.ERR_NOT_LOADED
NO_INDEX = b"no BWT loaded"
READ_ARGS = b"count_read_kmers needs 1 <= k <= min(64, read_len) and an output"
RAGGED_ARGS = b"count_ragged_read_kmers needs 1 <= k <= 64 and offsets"
SEARCH_COUNTERS = 16  # MSBWT_SEARCH_COUNTERS


@pytest.fixture
def L():
    return _lib.lib()


@pytest.fixture
def h(L):
    handle = L.msbwt_rle_new(8)
    assert handle
    yield handle
    L.msbwt_rle_free(handle)


def u64s(n):
    return (C.c_uint64 * n)()


def test_null_handle_is_rejected_everywhere(L):
    buf, out, out2 = (C.c_uint8 * 64)(), u64s(64), u64s(64)
    one = u64s(1)
    assert L.msbwt_rle_load_vector(None, buf, 4) == INVALID
    assert L.msbwt_rle_load_numpy_file(None, b"x.npy") == INVALID
    assert L.msbwt_rle_get_symbol_count(None, 1) == 0 and L.msbwt_rle_get_total_size(None) == 0
    assert L.msbwt_rle_count_kmers(None, buf, 4, 2, out) == INVALID
    assert L.msbwt_rle_count_kmer(None, buf, 4, one) == INVALID
    assert L.msbwt_rle_count_kmers_device(None, buf, 4, 2, out, None) == INVALID
    assert L.msbwt_rle_count_kmers_packed(None, out, 4, 2, out2, 64) == INVALID
    assert L.msbwt_rle_count_kmers_packed_device(None, out, 4, 2, out2, None) == INVALID
    assert L.msbwt_rle_constrain_ranges(None, buf, out, out2, 2, out, out2) == INVALID
    assert L.msbwt_rle_constrain_range(None, 1, 0, 1, out, out2) == INVALID
    assert L.msbwt_rle_constrain_ranges_device(None, buf, out, out2, 2, out, out2, None) == INVALID
    assert L.msbwt_rle_kmer_ranges(None, buf, 4, 2, out, out2) == INVALID
    assert L.msbwt_rle_kmer_ranges_device(None, buf, 4, 2, out, out2, None) == INVALID
    assert L.msbwt_rle_count_kmer_extensions(None, buf, 4, 2, out) == INVALID
    assert L.msbwt_rle_count_kmer_extensions_device(None, buf, 4, 2, out, None) == INVALID
    assert L.msbwt_rle_count_read_kmers(None, buf, 8, 2, 4, 0, out, out2) == INVALID
    assert L.msbwt_rle_count_read_kmers_device(None, buf, 8, 2, 4, 0, out, out2, None) == INVALID
    assert L.msbwt_rle_count_ragged_read_kmers(None, buf, out, 1, 4, 0, out, out2, one) == INVALID
    assert L.msbwt_rle_device_status(None, None) == INVALID
    assert L.msbwt_rle_replicate(None, 0) is None
    assert L.msbwt_rle_count_kmers_allgather_device(None, C.c_void_p(1), buf, 4, 2, out, out2, 64, 64, 1, None) == INVALID
    assert L.msbwt_rle_allgather_counts(None, C.c_void_p(1), out, 2, out2, 64, None) == INVALID
    assert L.msbwt_rle_kmer_order_keys_device(None, buf, 4, 2, out, None) == INVALID
    assert L.msbwt_rle_batch_order_for(None, 31, 10) == INVALID
    assert L.msbwt_rle_search_kernel_for(None, 31) == INVALID
    assert L.msbwt_rle_probe_line_rate(None, 0, C.byref(C.c_double())) == INVALID
    assert L.msbwt_rle_search_counters(None, out, None) == INVALID
    assert L.msbwt_rle_sparse_table_info(None, u64s(_lib.SPARSE_INFO_WORDS)) == INVALID
    assert L.msbwt_rle_table_info(None, out, out, out) == INVALID
    assert L.msbwt_rle_kernel_time_ms(None, None, None) == INVALID
    assert L.msbwt_rle_download_sparse_table(None, None, 0, None, 0) == _lib.SIZE_MAX
    assert L.msbwt_rle_download_blocks(None, None, 0) == _lib.SIZE_MAX
    for setter, value in (("table_depth", 8), ("pair_index", 1), ("pair_stride", 96), ("presence_filter", 0), ("table_packed", 1),
                          ("table_side", 0), ("sparse_table", 20), ("sparse_tiers", 1), ("sparse_second", 0), ("query_length", 31),
                          ("line_streaming", 1), ("batch_order", 1), ("search_counters", 1), ("block_format", 1), ("search_kernel", 2),
                          ("kernel_timing", 1)):
        assert getattr(L, "msbwt_rle_set_" + setter)(None, value) == INVALID, setter
    assert L.msbwt_rle_set_memory_budget(None, 1 << 30) == INVALID
    for getter in ("table_depth", "pair_index", "pair_stride", "table_packed", "sparse_table", "sparse_tiers", "query_length",
                   "line_streaming", "batch_order", "presence_filter", "block_format", "search_kernel"):
        assert getattr(L, "msbwt_rle_get_" + getter)(None) == 0, getter
    assert L.msbwt_rle_get_memory_budget(None) == 0 and L.msbwt_rle_device_bytes(None) == 0
    assert L.msbwt_rle_device_ordinal(None) == -1
    assert L.msbwt_rle_last_error(None) == b"null handle"


def test_unloaded_handle_queries_report_not_loaded(L, h):
    buf, out, out2 = (C.c_uint8 * 64)(), u64s(64), u64s(64)
    one = u64s(1)
    calls = {
        "count_kmers": lambda: L.msbwt_rle_count_kmers(h, buf, 4, 2, out),
        "count_kmer": lambda: L.msbwt_rle_count_kmer(h, buf, 4, one),
        "count_kmers_device": lambda: L.msbwt_rle_count_kmers_device(h, buf, 4, 2, out, None),
        "count_kmers_packed": lambda: L.msbwt_rle_count_kmers_packed(h, out, 4, 2, out2, 64),
        "count_kmers_packed_device": lambda: L.msbwt_rle_count_kmers_packed_device(h, out, 4, 2, out2, None),
        "constrain_ranges": lambda: L.msbwt_rle_constrain_ranges(h, buf, out, out2, 2, out, out2),
        "constrain_range": lambda: L.msbwt_rle_constrain_range(h, 1, 0, 1, out, out2),
        "constrain_ranges_device": lambda: L.msbwt_rle_constrain_ranges_device(h, buf, out, out2, 2, out, out2, None),
        "kmer_ranges": lambda: L.msbwt_rle_kmer_ranges(h, buf, 4, 2, out, out2),
        "kmer_ranges_device": lambda: L.msbwt_rle_kmer_ranges_device(h, buf, 4, 2, out, out2, None),
        "count_kmer_extensions": lambda: L.msbwt_rle_count_kmer_extensions(h, buf, 4, 2, out),
        "count_kmer_extensions_device": lambda: L.msbwt_rle_count_kmer_extensions_device(h, buf, 4, 2, out, None),
        "count_read_kmers": lambda: L.msbwt_rle_count_read_kmers(h, buf, 8, 2, 4, 0, out, out2),
        "count_read_kmers_device": lambda: L.msbwt_rle_count_read_kmers_device(h, buf, 8, 2, 4, 0, out, out2, None),
        "count_kmers_allgather_device": lambda: L.msbwt_rle_count_kmers_allgather_device(h, C.c_void_p(1), buf, 4, 2, out, out2, 64, 64, 1, None),
        "probe_line_rate": lambda: L.msbwt_rle_probe_line_rate(h, 0, C.byref(C.c_double())),
    }
    for name, call in calls.items():
        assert L.msbwt_rle_kmer_order_keys_device(h, buf, 0, 2, out, None) == INVALID  # another text first: each call sets its own
        assert call() == NOT_LOADED, name
        assert L.msbwt_rle_last_error(h) == NO_INDEX, name
    # the same with n = 0: nothing to do, but the missing index is still reported
    assert L.msbwt_rle_count_kmers(h, None, 4, 0, None) == NOT_LOADED
    assert L.msbwt_rle_count_kmers_packed(h, None, 4, 0, None, 64) == NOT_LOADED
    assert L.msbwt_rle_constrain_ranges(h, None, None, None, 0, None, None) == NOT_LOADED
    assert L.msbwt_rle_kmer_ranges(h, None, 4, 0, None, None) == NOT_LOADED
    assert L.msbwt_rle_count_kmer_extensions(h, None, 4, 0, None) == NOT_LOADED
    # what returns without an index and without touching a device
    assert L.msbwt_rle_replicate(h, 0) is None and L.msbwt_rle_last_error(h) == NO_INDEX
    assert L.msbwt_rle_batch_order_for(h, 31, 10) == INVALID
    assert L.msbwt_rle_search_kernel_for(h, 31) == INVALID
    assert L.msbwt_rle_download_sparse_table(h, None, 0, None, 0) == _lib.SIZE_MAX
    assert L.msbwt_rle_download_blocks(h, None, 0) == _lib.SIZE_MAX
    assert L.msbwt_rle_device_status(h, None) == OK  # no status block yet: nothing can have been flagged
    counters = u64s(SEARCH_COUNTERS)
    for i in range(SEARCH_COUNTERS):
        counters[i] = 7
    assert L.msbwt_rle_search_counters(h, counters, None) == OK and list(counters) == [0] * SEARCH_COUNTERS
    info = u64s(_lib.SPARSE_INFO_WORDS)
    for i in range(_lib.SPARSE_INFO_WORDS):
        info[i] = 9
    assert L.msbwt_rle_sparse_table_info(h, info) == OK and list(info) == [0] * _lib.SPARSE_INFO_WORDS
    assert L.msbwt_rle_sparse_table_info(h, None) == INVALID
    lines, esc, side = C.c_uint64(5), C.c_uint64(5), C.c_uint64(5)
    assert L.msbwt_rle_table_info(h, C.byref(lines), C.byref(esc), C.byref(side)) == OK
    assert (lines.value, esc.value, side.value) == (0, 0, 0)
    assert L.msbwt_rle_get_total_size(h) == 0 and L.msbwt_rle_get_symbol_count(h, 1) == 0 and L.msbwt_rle_device_bytes(h) == 0
    assert L.msbwt_rle_get_typical_range_width(h) == -1.0


def test_unloaded_handle_null_buffers_report_the_missing_index_first(L, h):
    """The query entry points check for an index before their buffers (count_read_kmers is the exception: arguments first)."""
    buf = (C.c_uint8 * 64)()
    out = u64s(64)
    assert L.msbwt_rle_count_kmers(h, None, 4, 3, None) == NOT_LOADED
    assert L.msbwt_rle_count_kmers_device(h, None, 4, 3, None, None) == NOT_LOADED
    assert L.msbwt_rle_count_kmers_packed(h, None, 4, 3, None, 64) == NOT_LOADED
    assert L.msbwt_rle_count_kmers_packed_device(h, None, 4, 3, None, None) == NOT_LOADED
    assert L.msbwt_rle_constrain_ranges(h, None, None, None, 3, None, None) == NOT_LOADED
    assert L.msbwt_rle_constrain_ranges_device(h, None, None, None, 3, None, None, None) == NOT_LOADED
    assert L.msbwt_rle_kmer_ranges(h, None, 4, 3, None, None) == NOT_LOADED
    assert L.msbwt_rle_kmer_ranges_device(h, None, 4, 3, None, None, None) == NOT_LOADED
    assert L.msbwt_rle_count_kmer_extensions(h, None, 4, 3, None) == NOT_LOADED
    assert L.msbwt_rle_count_kmer_extensions_device(h, None, 4, 3, None, None) == NOT_LOADED
    assert L.msbwt_rle_count_read_kmers_device(h, None, 8, 3, 4, 0, None, None, None) == NOT_LOADED
    assert L.msbwt_rle_count_kmers_allgather_device(h, None, None, 0, 3, None, None, 48, 8, 0, None) == NOT_LOADED
    assert L.msbwt_rle_last_error(h) == NO_INDEX
    # out-of-range arguments on an unloaded handle: the index is checked first ...
    assert L.msbwt_rle_count_kmers_packed(h, out, 65, 2, out, 64) == NOT_LOADED
    assert L.msbwt_rle_count_kmers_packed(h, out, 4, 2, out, 48) == NOT_LOADED
    assert L.msbwt_rle_count_kmers_packed_device(h, out, 65, 2, out, None) == NOT_LOADED
    assert L.msbwt_rle_count_read_kmers_device(h, buf, 8, 2, 0, 0, out, None, None) == NOT_LOADED
    assert L.msbwt_rle_count_read_kmers_device(h, buf, 8, 2, 9, 0, out, None, None) == NOT_LOADED
    # ... except by count_read_kmers, which checks its arguments before the index
    for k, read_len, fwd, rc, reads in ((0, 8, out, None, buf), (9, 8, out, None, buf), (65, 100, out, None, buf), (4, 8, None, None, buf),
                                        (4, 8, out, None, None)):
        assert L.msbwt_rle_count_read_kmers(h, reads, read_len, 2, k, 0, fwd, rc) == INVALID, (k, read_len)
        assert L.msbwt_rle_last_error(h) == READ_ARGS
    assert L.msbwt_rle_count_read_kmers(h, None, 8, 0, 4, 0, out, None) == NOT_LOADED  # no reads, no buffer needed
    assert L.msbwt_rle_count_read_kmers(h, buf, 8, 2, 8, 1, None, out) == NOT_LOADED
    assert L.msbwt_rle_last_error(h) == NO_INDEX


def test_multi_replica_entry_points(L, h):
    buf = (C.c_uint8 * 64)()
    out = u64s(64)
    Arr = C.c_void_p * 2
    two = Arr(h, h)
    with_null = Arr(h, None)
    assert L.msbwt_rle_count_kmers_multi(None, 2, buf, 4, 2, out) == INVALID
    assert L.msbwt_rle_count_kmers_multi(two, 0, buf, 4, 2, out) == INVALID
    assert L.msbwt_rle_count_kmers_multi(with_null, 2, buf, 4, 2, out) == INVALID
    assert L.msbwt_rle_count_kmers_multi(two, 2, buf, 4, 2, None) == INVALID
    assert L.msbwt_rle_count_kmers_multi(two, 1, buf, 4, 40, out) == NOT_LOADED
    assert L.msbwt_rle_count_read_kmers_multi(two, 1, buf, 8, 2, 0, 0, out, None) == INVALID
    assert L.msbwt_rle_count_read_kmers_multi(two, 1, buf, 8, 2, 9, 0, out, None) == INVALID
    assert L.msbwt_rle_count_read_kmers_multi(with_null, 2, buf, 8, 2, 4, 0, out, None) == INVALID
    assert L.msbwt_rle_count_read_kmers_multi(two, 1, buf, 8, 2, 4, 0, out, None) == NOT_LOADED
    assert L.msbwt_rle_count_kmers_multi_device(None, 1, buf, 4, 2, out) == INVALID
    assert L.msbwt_rle_count_kmers_multi_device(with_null, 2, buf, 4, 2, out) == INVALID
    assert L.msbwt_rle_count_kmers_multi_device(two, 1, buf, 4, 2, None) == INVALID
    assert L.msbwt_rle_count_kmers_multi_device(two, 1, buf, 4, 2, out) == NOT_LOADED
    assert L.msbwt_rle_last_error(h) == NO_INDEX


def test_argument_checks_without_an_index(L, h):
    buf = (C.c_uint8 * 64)()
    out = u64s(64)
    fake = C.c_void_p(1)
    # order keys: arguments only (no index needed)
    assert L.msbwt_rle_kmer_order_keys_device(h, buf, 0, 2, out, None) == INVALID
    assert L.msbwt_rle_last_error(h) == b"order keys need 1 <= k and buffers"
    assert L.msbwt_rle_kmer_order_keys_device(h, None, 4, 2, out, None) == INVALID
    assert L.msbwt_kmer_order_keys(buf, 0, 2, out) == INVALID
    assert L.msbwt_kmers_pack_2bit(buf, 65, 1, out) == INVALID and L.msbwt_kmers_pack_2bit(buf, 0, 1, out) == INVALID
    # all-gather of counts: arguments only
    for comm, n, bits in ((None, 0, 64), (fake, 0, 48), (fake, 5, 64)):
        assert L.msbwt_rle_allgather_counts(h, comm, None, n, None, bits, None) == INVALID
        assert L.msbwt_rle_last_error(h).startswith(b"allgather_counts needs a communicator")
    # line-rate probe: arguments before the lock and the index
    assert L.msbwt_rle_probe_line_rate(h, 4, C.byref(C.c_double())) == INVALID
    assert L.msbwt_rle_probe_line_rate(h, 0, None) == INVALID
    # ragged reads
    offs = u64s(4)
    for i, v in enumerate((0, 10, 20, 25)):
        offs[i] = v
    win = C.c_uint64(0)
    assert L.msbwt_rle_count_ragged_read_kmers(h, buf, offs, 3, 0, 0, out, None, C.byref(win)) == INVALID
    assert L.msbwt_rle_last_error(h) == RAGGED_ARGS
    assert L.msbwt_rle_count_ragged_read_kmers(h, buf, offs, 3, 65, 0, out, None, C.byref(win)) == INVALID
    assert L.msbwt_rle_count_ragged_read_kmers(h, buf, None, 3, 4, 0, out, None, C.byref(win)) == INVALID
    assert L.msbwt_rle_count_ragged_read_kmers(h, None, offs, 3, 4, 0, out, None, C.byref(win)) == INVALID
    bad = u64s(3)
    bad[0], bad[1], bad[2] = 0, 10, 5
    assert L.msbwt_rle_count_ragged_read_kmers(h, buf, bad, 2, 4, 0, out, None, C.byref(win)) == INVALID
    assert L.msbwt_rle_last_error(h) == b"read offsets must not decrease"
    # only the window count: answered without an index (reads of 10, 10 and 5 symbols at k = 6: 5 + 5 + 0)
    L.msbwt_rle_count_kmers(h, None, 4, 1, None)
    assert L.msbwt_rle_count_ragged_read_kmers(h, buf, offs, 3, 6, 0, None, None, C.byref(win)) == OK
    assert win.value == 10
    assert L.msbwt_rle_last_error(h) == NO_INDEX  # (OK leaves the text of the last failure)
    assert L.msbwt_rle_count_ragged_read_kmers(h, buf, offs, 3, 11, 0, None, None, C.byref(win)) == OK and win.value == 0
    assert L.msbwt_rle_count_ragged_read_kmers(h, None, None, 0, 4, 0, None, None, C.byref(win)) == OK and win.value == 0
    # with an output the index is needed -- even when there are no windows at all
    win.value = 99
    assert L.msbwt_rle_count_ragged_read_kmers(h, buf, offs, 3, 6, 0, out, None, C.byref(win)) == NOT_LOADED and win.value == 10
    assert L.msbwt_rle_count_ragged_read_kmers(h, buf, offs, 3, 11, 0, None, out, C.byref(win)) == NOT_LOADED and win.value == 0
    assert L.msbwt_rle_count_ragged_read_kmers(h, buf, offs, 3, 6, 0, out, None, None) == NOT_LOADED
    # loading: arguments before anything else
    assert L.msbwt_rle_load_vector(h, None, 4) == INVALID
    assert L.msbwt_rle_load_numpy_file(h, None) == INVALID
    assert L.msbwt_rle_load_numpy_file(h, b"/nonexistent/dir/no.npy") == _lib.ERR_IO
    assert L.msbwt_rle_last_error(h)
    assert L.msbwt_rle_constrain_range(h, 1, 0, 1, None, out) == INVALID
    assert L.msbwt_rle_count_kmer(h, buf, 4, None) == INVALID


def test_setters_on_an_unloaded_handle(L, h):
    """Out-of-range values are refused without a text; accepted ones are recorded and reported back without a device."""
    L.msbwt_rle_count_kmers(h, None, 4, 1, None)  # puts a known text on the handle
    rejected = (("table_depth", 17), ("pair_index", -2), ("pair_index", 2), ("pair_stride", 64), ("pair_stride", 1), ("presence_filter", 2),
                ("presence_filter", -2), ("table_packed", 2), ("table_packed", -2), ("table_side", -1), ("table_side", 2), ("sparse_table", 15),
                ("sparse_table", -2), ("sparse_table", 32), ("sparse_tiers", 2), ("sparse_tiers", -2), ("sparse_second", 1), ("sparse_second", -2),
                ("query_length", -1), ("line_streaming", 2), ("line_streaming", -2), ("batch_order", 2), ("batch_order", -2), ("block_format", 2),
                ("block_format", -1), ("search_kernel", 3), ("search_kernel", -1))
    for setter, value in rejected:
        assert getattr(L, "msbwt_rle_set_" + setter)(h, value) == INVALID, (setter, value)
    assert L.msbwt_rle_last_error(h) == NO_INDEX
    accepted = (("table_depth", 12), ("table_depth", -1), ("pair_index", 0), ("pair_index", 1), ("pair_index", -1), ("pair_stride", 96),
                ("pair_stride", 128), ("pair_stride", 0), ("presence_filter", 0), ("presence_filter", 1), ("table_packed", 1), ("table_packed", 0),
                ("table_side", 0), ("table_side", 1), ("sparse_table", 0), ("sparse_table", 20), ("sparse_table", -1), ("sparse_tiers", 1),
                ("sparse_tiers", 1), ("sparse_tiers", 0), ("sparse_second", 0), ("sparse_second", -1), ("query_length", 31), ("query_length", 0),
                ("line_streaming", 1), ("batch_order", 1), ("search_counters", 1), ("search_counters", 0), ("block_format", 1), ("search_kernel", 2),
                ("kernel_timing", 1), ("kernel_timing", 0))
    for setter, value in accepted:
        assert getattr(L, "msbwt_rle_set_" + setter)(h, value) == OK, (setter, value)
    assert L.msbwt_rle_set_memory_budget(h, 1 << 34) == OK and L.msbwt_rle_get_memory_budget(h) == 1 << 34
    assert L.msbwt_rle_set_memory_budget(h, 0) == OK and L.msbwt_rle_get_memory_budget(h) == 0
    assert L.msbwt_rle_last_error(h) == NO_INDEX
    # the wishes are recorded ...
    assert L.msbwt_rle_set_query_length(h, 27) == OK and L.msbwt_rle_get_query_length(h) == 27
    assert L.msbwt_rle_get_batch_order(h) == 1
    assert L.msbwt_rle_get_search_kernel(h) == 2
    assert L.msbwt_rle_get_block_format(h) == 1
    # ... while what reports the index in HBM reports none
    assert L.msbwt_rle_get_table_depth(h) == 0 and L.msbwt_rle_get_table_packed(h) == 0
    assert L.msbwt_rle_get_pair_index(h) == 0 and L.msbwt_rle_get_pair_stride(h) == 0
    assert L.msbwt_rle_get_presence_filter(h) == 0
    assert L.msbwt_rle_get_sparse_table(h) == 0 and L.msbwt_rle_get_sparse_tiers(h) == 0
    assert L.msbwt_rle_get_line_streaming(h) == 0
    assert L.msbwt_rle_device_bytes(h) == 0
