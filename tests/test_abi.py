"""The C-ABI library loads and exports every symbol include/rpcc_hip.h declares (no GPU needed)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    import rpcc_amd  # noqa: F401
    from rpcc_amd import _lib
    return _lib


def test_header_symbols_exported(built):
    hdr = open(os.path.join(ROOT, "include", "rpcc_hip.h")).read()
    declared = sorted(set(re.findall(r"\b(rpcc_[a-z0-9_]+)\s*\(", hdr)))
    assert len(declared) >= 12
    lib = ctypes.CDLL(built.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name
    assert sorted(built.exported_symbols()) == declared


def test_version_and_workspace(built):
    lib = built.lib()
    assert lib.rpcc_version() == built.ABI_VERSION
    assert lib.rpcc_workspace_bytes(256, 64 * 2048, 100, 0) > 0
    assert lib.rpcc_workspace_bytes(0, 64 * 2048, 100, 0) == 0


# Workspace sizes the library returned before its workspaces were carved by layout functions (csrc/rpcc_hip.hip: Carve and the *_layout
# functions), over B x geometry (x M (x total_points)) in the loop order of test_workspace_sizes_are_pinned.  An odd P is included.
_SIZE_BS = (1, 3, 129, 256)
_SIZE_GEOMS = ((16, 1800), (32, 2250), (64, 2000), (64, 2048), (80, 2000), (31, 997))
_SIZE_MS = (1, 100, 254)
_WS = [
    853952, 1428416, 2003136, 861888, 1436352, 2011072, 877760, 1452224, 2026944, 1818080, 4690912, 7564000, 1836768, 4709600, 7582688,
    1874144, 4746976, 7620064, 3035904, 8132352, 13277952, 3068416, 8164864, 13310464, 3133440, 8229888, 13375488, 3102720, 8346624,
    13590528, 3136000, 8379904, 13623808, 3202560, 8446464, 13690368, 3756672, 13349248, 22942080, 3797376, 13389952, 22982784, 3878784,
    13471360, 23064192, 899792, 1515728, 2131920, 908240, 1524176, 2140368, 925136, 1541072, 2157264, 1859392, 3583296, 5306944, 1883200,
    3607104, 5330752, 1930816, 3654720, 5378368, 3714976, 12333728, 20952480, 3771040, 12389792, 21008544, 3883168, 12501920, 21120672,
    6024448, 21362944, 36750592, 6121984, 21460480, 36848128, 6317056, 21655552, 37043200, 6151168, 21882880, 37614848, 6251008, 21982720,
    37714688, 6450688, 22182400, 37914368, 7419008, 36196992, 64974976, 7541120, 36319104, 65097088, 7785344, 36563328, 65341312, 1946344,
    3794408, 5642472, 1971688, 3819752, 5667816, 2022376, 3870440, 5718504, 65211328, 139528384, 213845184, 66235072, 140552128, 214868928,
    68282560, 142599616, 216916416, 123231712, 494816480, 866401504, 125642464, 497227232, 868812256, 130463968, 502048736, 873633760,
    194315008, 854899456, 1515533056, 198509056, 859093504, 1519727104, 206897152, 867481600, 1528115200, 198215680, 874679296, 1551142912,
    202508800, 878972416, 1555436032, 211095040, 887558656, 1564022272, 238145152, 1476777856, 2715410560, 243395968, 1482028672,
    2720661376, 253897600, 1492530304, 2731163008, 67885776, 147622096, 227383248, 68975568, 148711888, 228473040, 71155152, 150891472,
    230652624, 129065728, 276550400, 424035328, 131097344, 278582016, 426066944, 135160576, 282645248, 430130176, 243696640, 981120512,
    1718544640, 248480768, 985904640, 1723328768, 258049024, 995472896, 1732897024, 384099584, 1695075584, 3006051584, 392422656,
    1703398656, 3014374656, 409068800, 1720044800, 3031020800, 391804160, 1734243584, 3076683008, 400323840, 1742763264, 3085202688,
    417363200, 1759802624, 3102242048, 470702336, 2928782336, 5386862336, 481122560, 2939202560, 5397282560, 501963008, 2960043008,
    5418123008, 134348228, 292613572, 450879172, 136510916, 294776260, 453041860, 140836292, 299101636, 457367236,
]

_WS_GENERAL = [
    1430720, 2005184, 2579904, 1439168, 2013632, 2588352, 1456064, 2030528, 2605248, 3258848, 6131680, 9004768, 3278048, 6150880, 9023968,
    3316448, 6189280, 9062368, 5596672, 10693120, 15838720, 5629696, 10726144, 15871744, 5695744, 10792192, 15937792, 5724928, 10968832,
    16212736, 5758720, 11002624, 16246528, 5826304, 11070208, 16314112, 6957440, 16550016, 26142848, 6998656, 16591232, 26184064, 7081088,
    16673664, 26266496, 1518720, 2134656, 2750848, 1527680, 2143616, 2759808, 1545600, 2161536, 2777728, 3588160, 5312064, 7035712, 3614016,
    5337920, 7061568, 3665216, 5389120, 7112768, 8035744, 16654496, 25273248, 8093856, 16712608, 25331360, 8209568, 16828320, 25447072,
    13705216, 29043712, 44431360, 13804800, 29143296, 44530944, 14003456, 29341952, 44729600, 14016256, 29747968, 45479936, 14118144,
    29849856, 45581824, 14321408, 30053120, 45785088, 17019776, 45797760, 74575744, 17143936, 45921920, 74699904, 17391744, 46169728,
    74947712, 3801592, 5649656, 7497720, 3828984, 5677048, 7525112, 3883256, 5731320, 7579384, 139519168, 213836224, 288153024, 140644800,
    214961856, 289278656, 142851008, 217168064, 291484864, 308995552, 680580320, 1052165344, 311508192, 683092960, 1054677984, 316488416,
    688073184, 1059658208, 524558848, 1185143296, 1845776896, 528854784, 1189439232, 1850072832, 537401600, 1197986048, 1858619648,
    536385280, 1212848896, 1889312512, 540780288, 1217243904, 1893707520, 549525248, 1225988864, 1902452480, 650948992, 1889581696,
    3128214400, 656301696, 1894934400, 3133567104, 666962048, 1905594752, 3144227456, 147629696, 227366016, 307127168, 148821376, 228557696,
    308318848, 151159680, 230896000, 310657152, 276528128, 424012800, 571497728, 278762496, 426247168, 573732096, 283141120, 430625792,
    578110720, 612343040, 1349766912, 2087191040, 617329920, 1354753792, 2092177920, 627213568, 1364637440, 2102061568, 1039465984,
    2350441984, 3661417984, 1047991808, 2358967808, 3669943808, 1064953344, 2375929344, 3686905344, 1062899200, 2405338624, 3747778048,
    1071621632, 2414061056, 3756500480, 1088976384, 2431415808, 3773855232, 1289908736, 3747988736, 6206068736, 1300531712, 3758611712,
    6216691712, 1321687552, 3779767552, 6237847552, 292598468, 450863812, 609129412, 294963908, 453229252, 611494852, 299604676, 457870020,
    616135620,
]

_PROJECT_SCRATCH = [
    140120, 714696, 1289328, 337504, 3210384, 6083376, 561504, 5657920, 10803616, 573792, 5817696, 11061712, 714120, 10306776, 19899600,
    148552, 764560, 1380640, 419784, 2143512, 3867296, 1011968, 9630608, 18249360, 1683968, 17022384, 32410080, 1720832, 17452544, 33184368,
    2141784, 30919752, 59697888, 445080, 2293120, 4141232, 18038616, 92355592, 166672624, 43503200, 415088080, 786673072, 72399200,
    732983616, 1393617312, 73984352, 750447968, 1426911696, 92084616, 1330717272, 2569350096, 19125832, 98862320, 178623440, 35797264,
    183282064, 330766920, 86331664, 823755664, 1561179776, 143675664, 1454651664, 2765627776, 146821392, 1489260816, 2831700352, 182741264,
    2640821264, 5098901432, 37954832, 196220368, 354485944,
]

_PLANE_WS = [
    584448, 592384, 608256, 1459200, 1477888, 1515264, 2593024, 2625536, 2690560, 2655232, 2688512, 2755072, 3241216, 3281920, 3363328,
    627120, 635568, 652464, 1752320, 1776128, 1823744, 4376576, 4432640, 4544768, 7778048, 7875584, 8070656, 7964672, 8064512, 8264192,
    9722624, 9844736, 10088960, 1880336, 1905680, 1956368, 75330304, 76354048, 78401536, 188173312, 190584064, 195405568, 334436608,
    338630656, 347018752, 342461440, 346754560, 355340800, 418053376, 423304192, 433805824, 80832432, 81922224, 84101808, 149491968,
    151523584, 155586816, 373428480, 378212608, 387780864, 663687424, 672010496, 688656640, 679612672, 688132352, 705171712, 829624576,
    840044800, 860885248, 160410880, 162573568, 166898944,
]

_CODEC_WS = [
    8564, 16500, 32372, 19484, 38172, 75548, 33524, 66036, 131060, 34304, 67584, 134144, 41844, 82548, 163956, 9084, 17532, 34428, 24668,
    48476, 96092, 57428, 113492, 225620, 99548, 197084, 392156, 101888, 201728, 401408, 124508, 246620, 490844, 26228, 51572, 102260,
    1041268, 2065012, 4112500, 2449948, 4860700, 9682204, 4261108, 8455156, 16843252, 4361728, 8654848, 17241088, 5334388, 10585204,
    21086836, 1108348, 2198140, 4377724, 2065664, 4097280, 8160512, 4861184, 9645312, 19213568, 8455424, 16778496, 33424640, 8655104,
    17174784, 34214144, 10585344, 21005568, 41846016, 2198784, 4361472, 8686848,
]

_FPS_TABLE = [
    5472, 13632, 24192, 24576, 30240, 6144, 16416, 40896, 72576, 73728, 90720, 18432, 705888, 1758528, 3120768, 3170304, 3900960, 792576,
    1400832, 3489792, 6193152, 6291456, 7741440, 1572864,
]


def test_workspace_sizes_are_pinned(built):
    """The exported sizes equal the recorded ones.  The one exception is rpcc_workspace_bytes_general: its plane area starts after the FPS
    tile table rounded up to 256 bytes, which the size now counts -- exactly that round-up more, always under 256 bytes."""
    lib = built.lib()
    ws, gen, proj, plane, codec, fps = (iter(v) for v in (_WS, _WS_GENERAL, _PROJECT_SCRATCH, _PLANE_WS, _CODEC_WS, _FPS_TABLE))
    for B in _SIZE_BS:
        for H, W in _SIZE_GEOMS:
            P = H * W
            assert lib.rpcc_fps_table_bytes(B, H, W) == next(fps)
            for t in (0, B * P, 2 * B * P + 7):
                assert lib.rpcc_project_scratch_bytes(t, B, P) == next(proj), (B, P, t)
            tab = B * 12 * ((P + 31) // 32 + 4096) * 4       # the tile-table bound of a batch workspace
            for M in _SIZE_MS:
                assert lib.rpcc_plane_workspace_bytes(B, P, M) == next(plane), (B, P, M)
                assert lib.rpcc_codec_workspace_bytes(B, P, M) == next(codec), (B, P, M)
                for t in (0, B * P, 2 * B * P + 7):
                    assert lib.rpcc_workspace_bytes(B, P, M, t) == next(ws), (B, P, M, t)
                    grown = lib.rpcc_workspace_bytes_general(B, P, M, t) - next(gen)
                    assert grown == -tab % 256 and 0 <= grown < 256, (B, P, M, t, grown)
                    assert lib.rpcc_wide_workspace_bytes(B, P, M, t) >= lib.rpcc_workspace_bytes_general(B, P, M, t)
    for v in (ws, gen, proj, plane, codec, fps):
        assert next(v, None) is None
    for M in (255, 1022):
        assert lib.rpcc_wide_workspace_bytes(3, 64 * 2048, M, 0) >= lib.rpcc_workspace_bytes_general(3, 64 * 2048, M, 0)


def test_argument_errors_do_not_crash(built):
    lib = built.lib()
    rc = lib.rpcc_fps_xyz(0, 10, 5, None, None, None, None)
    assert rc == -1 and b"bad argument" in lib.rpcc_last_error()


def test_unknown_batch_flags_are_refused(built):
    """rpcc_batch_io.flags takes the FPS bits only: 16 and 32 (the scanner-order projection bits of ABI 103) are an argument error,
    raised before anything touches the device (every pointer below is a host dummy that must never reach a kernel)."""
    lib = built.lib()
    dummy = ctypes.create_string_buffer(256)
    p = ctypes.addressof(dummy)
    geom = built.Geom(64, 2048, 6.2831855, 0.034906585, -0.43458698)
    for flags in (16, 32, 16 | 1):
        io = built.BatchIO(p, p, 1000, p, p, -1, None, p, p, p, p, p, p, p, p, p, flags, None, 0, 0.0, 0, None, None, None, 12)
        for name, extra in (("rpcc_compress_batch", ()), ("rpcc_compress_batch_stages", (1,)), ("rpcc_compress_batch_wide", ())):
            rc = getattr(lib, name)(ctypes.byref(io), 2, geom, 100, 0.1, 0.04, p, *extra, None)
            assert rc == -1 and b"flags" in lib.rpcc_last_error(), (name, flags, rc, lib.rpcc_last_error())


def test_product_never_imports_oracle():
    """The oracle is test infrastructure: nothing under r-pcc_amd/ may import, link or load it."""
    bad = re.compile(r"(^|\n)\s*(from|import)\s+oracle\b|liborpcc|oracle/_ref|oracle\.oracle")
    for dp, _, fs in os.walk(os.path.join(ROOT, "r-pcc_amd")):
        for f in fs:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                assert not bad.search(open(os.path.join(dp, f)).read()), (dp, f)


def test_cluster_num_limits_are_named():
    """The reference takes any cluster_num (cfgs/compressor.yaml:22; uint16 labels in the stream).  The batch front-end does too (above 254 through the
    uint16-label entries, up to 65 533); the mirror classes' per-stage entries keep labels in a byte and must refuse a larger value with the limit
    spelled out -- in the front-end, before anything touches the device -- not with a bare argument error."""
    import re
    import pytest
    import rpcc_amd  # noqa: F401
    from rpcc_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "rpcc_hip.h")).read()
    assert int(re.search(r"#define RPCC_MAX_CLUSTERS (\d+)", hdr).group(1)) == _lib.MAX_CLUSTERS == 254
    assert int(re.search(r"#define RPCC_MAX_CLUSTERS_WIDE (\d+)", hdr).group(1)) == _lib.MAX_CLUSTERS_WIDE == 65533
    assert ops.check_cluster_num(254) == 254 and ops.check_cluster_num(1) == 1 and ops.check_cluster_num(300) == 300 and ops.check_cluster_num(65533) == 65533
    assert not ops.is_wide(254) and ops.is_wide(255)
    for bad in (65534, 0):
        with pytest.raises(_lib.RpccError, match=r"cluster_num = %d.*<= 65533" % bad):
            ops.check_cluster_num(bad)
    for bad in (255, 300):
        with pytest.raises(_lib.RpccError, match=r"cluster_num = %d.*stage-by-stage.*<= 254.*uint8.*BatchCompressor" % bad):
            ops.check_cluster_num(bad, wide=False)
    # the stage seams that exist on uint16 labels (segmentation, point model, prediction, uniform quantiser): up to RPCC_MAX_CLUSTERS_MID
    assert int(re.search(r"#define RPCC_MAX_CLUSTERS_MID (\d+)", hdr).group(1)) == _lib.MAX_CLUSTERS_MID == 1022
    assert ops.check_cluster_num(300, stage="mid") == 300 and ops.check_cluster_num(1022, stage="mid") == 1022
    with pytest.raises(_lib.RpccError, match=r"cluster_num = 1023.*<= 1022.*BatchCompressor"):
        ops.check_cluster_num(1023, stage="mid")
    from rpcc_amd.pipeline import BatchCompressor
    with pytest.raises(_lib.RpccError, match="cluster_num = 70000"):
        BatchCompressor(None, cluster_num=70000)


def test_nothing_throws_across_the_abi(built):
    """include/rpcc_hip.h promises `int` status codes and no C++ exception across the boundary.  The only throwing operations in the library are the
    growth of its two host-side tables (kernel attributes, timer events): every push_back sits behind a reserve inside a try block or inside one
    itself, and the timer entry points answer with a status where there is no device at all (here) instead of terminating the process."""
    src = open(os.path.join(ROOT, "r-pcc_amd", "csrc", "rpcc_hip.hip")).read().splitlines()
    for i, line in enumerate(src):
        if "push_back(" in line and not line.lstrip().startswith("//"):
            ctx = "\n".join(src[max(0, i - 14):i + 1])
            assert "try {" in ctx, "push_back outside a try block / reserve: line %d" % (i + 1)
    lib = built.lib()
    lib.rpcc_timer_create.restype = ctypes.c_void_p
    t = ctypes.c_void_p(lib.rpcc_timer_create())
    assert t.value
    assert lib.rpcc_timer_reserve(t, (1 << 20) + 1) == -1            # RPCC_ERR_ARG
    rc = lib.rpcc_timer_reserve(t, 4)                                # no device here: a HIP status, not an exception (0 on a GPU box)
    assert rc in (0, -2), rc
    lib.rpcc_timer_destroy.argtypes = [ctypes.c_void_p]
    lib.rpcc_timer_destroy(t)


def test_a_failed_collect_frees_its_ring_slot():
    """pipeline.BatchCompressor keeps SLOTS buffer sets per batch size; a collect() that raises (stream error, host OOM in a copy) or a submit()
    whose caller gives up (discard) must free the slot, or the ring is exhausted after SLOTS such events."""
    import rpcc_amd  # noqa: F401
    from rpcc_amd.pipeline import BatchCompressor

    class Buf:
        in_flight = True

    class BadStream:
        def synchronize(self):
            raise RuntimeError("stream error")

    bc = object.__new__(BatchCompressor)
    b = Buf()
    with pytest.raises(RuntimeError, match="stream error"):
        bc.collect(dict(buf=b, stream=BadStream()))
    assert b.in_flight is False
    b.in_flight = True
    with pytest.raises(RuntimeError, match="stream error"):
        bc.discard(dict(buf=b, stream=BadStream()))
    assert b.in_flight is False


def test_cpu_pinning_only_with_explicit_local_ranks(monkeypatch):
    """utils.pin_rank_cpus slices the host's CPUs by LOCAL_RANK: only when the launcher named LOCAL_RANK and LOCAL_WORLD_SIZE, and not when the
    process already runs on a subset of the machine (bound by its launcher)."""
    import rpcc_amd  # noqa: F401
    from rpcc_amd import utils
    for k in ("LOCAL_RANK", "LOCAL_WORLD_SIZE", "RPCC_NO_AFFINITY", "RPCC_FORCE_AFFINITY"):
        monkeypatch.delenv(k, raising=False)
    assert utils.local_rank_env() is None
    monkeypatch.setenv("LOCAL_RANK", "1")
    assert utils.local_rank_env() is None
    monkeypatch.setenv("LOCAL_WORLD_SIZE", "4")
    assert utils.local_rank_env() == (1, 4)
    got = {}
    monkeypatch.setattr(os, "cpu_count", lambda: 16)
    monkeypatch.setattr(os, "sched_getaffinity", lambda pid: set(range(16)), raising=False)
    monkeypatch.setattr(os, "sched_setaffinity", lambda pid, cpus: got.update(cpus=list(cpus)), raising=False)
    assert utils.pin_rank_cpus(1, 4) == [4, 5, 6, 7] and got["cpus"] == [4, 5, 6, 7]
    assert utils.pin_rank_cpus(4, 4) is None                       # a rank outside its local world
    monkeypatch.setattr(os, "sched_getaffinity", lambda pid: set(range(4, 8)), raising=False)
    got.clear()
    assert utils.pin_rank_cpus(1, 4) is None and not got           # already bound to 4 of 16 CPUs: left alone
    monkeypatch.setenv("RPCC_FORCE_AFFINITY", "1")
    assert utils.pin_rank_cpus(1, 4) == [5]
