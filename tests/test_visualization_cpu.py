"""CPU-side checks of the stored-results path (csrc/flow_render.hip, hip.flow_image / flow_submission / event_image,
utils.visualization, utils.png): the numpy restatement the GPU tests compare against IS the reference (byte for byte on the fixture
the reference itself produced), the PNG codec round-trips, the three entry points are declared, exported and bound and refuse their
arguments before any launch, and the Python surface refuses what it cannot serve without touching a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import vis_cases as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sdf_flow_image_workspace_bytes", "sdf_flow_image_fwd", "sdf_flow_submission_fwd", "sdf_event_image_fwd")
E_NULL, E_SHAPE, E_DTYPE, E_ALIGN = -1, -2, -3, -4


@pytest.fixture(scope="module")
def lib():
    from sdformerflow_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return hip.lib()


@pytest.fixture(scope="module")
def golden():
    return np.load(V.GOLDEN)


# -- the restatement is the reference ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", V.FLOW_FIXTURES)
def test_flow_restatement_equals_the_reference(golden, name):
    flow = golden[f"flow/{name}"]
    assert np.array_equal(V.flow_image_ref(flow), golden[f"flow_img/{name}"])
    assert np.array_equal(V.submission_ref(flow), golden[f"sub/{name}"])


def test_flow_fixture_holds_its_edge_cases(golden):
    """What the cases are there for: a range of 0 leaves the value undivided (black), and a hue of exactly 1.0 (sector index 6) and
    of exactly 0.0 both fold to case 0 - pure red scaled by the value."""
    assert not golden["flow_img/const"].any() and not golden["flow_img/zero"].any()
    f = golden["flow/hue_edges"]
    for row in (0, 1):
        h = (np.arctan2(f[1, row, :5], f[0, row, :5]) + np.float32(np.pi)) * np.float32(1.0 / np.pi / 2.0)
        assert np.all(h == (1.0, 0.0)[row])
        px = golden["flow_img/hue_edges"][row, :5]
        assert px[:, 0].any() and not px[:, 1:].any()           # (the pixel of the smallest magnitude is black)


@pytest.mark.parametrize("name", V.EVENT_FIXTURES)
def test_event_restatement_equals_the_reference(golden, name):
    """The float image is the reference's; the bytes follow the stated rounding (nearest, halves to even) in the file's RGB order."""
    counts = golden[f"events/{name}"]
    img = V.event_float_image_ref(counts)
    assert np.array_equal(img, golden[f"events_img/{name}"])
    got = V.event_image_ref(counts)
    want = golden[f"events_img/{name}"][..., ::-1] * 255.0
    assert got.dtype == np.uint8 and np.all(np.abs(got - want) <= 0.5)
    ties = np.abs(got - want) == 0.5
    assert np.all(got[ties] % 2 == 0)
    assert not got[..., 2].any()                                # blue stays empty


def test_event_fixture_holds_its_branches(golden):
    s = golden["events/sparse"]
    assert (s != 0).mean() < 0.01 and np.percentile(s[0], 99) == 0 and np.percentile(s[1], 99) == 0
    assert np.array_equal(golden["events_img/sparse"][..., 1], np.clip(s[0], 0, 1))          # un-normalised: clipped only
    q = golden["events/posmin_eq_max"]
    assert np.percentile(q[0], 1) == max(np.percentile(q[0], 99), np.percentile(q[1], 99))
    assert np.all(golden["events_img/posmin_eq_max"][..., 1] == 1.0)
    assert np.array_equal(np.rint(np.array([0.5, 1.5, 2.5, 254.5])), [0, 2, 2, 254])         # np.rint is the stated rounding


def test_event_counts_restatement_modes():
    v = V.random_voxel(1, 10, 9, 11, seed=5)[0]
    split = np.stack([np.maximum(v, 0), np.maximum(-v, 0)], 1)
    assert np.array_equal(V.event_counts_ref(v), V.event_counts_ref(split))
    assert np.array_equal(V.event_counts_ref(v, (1, 3, 5, 6)), V.event_counts_ref(v)[:, 1:6, 3:9])


# -- PNG ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,shape", [(np.uint8, (5, 7, 3)), (np.uint8, (1, 1, 3)), (np.uint16, (6, 4, 3)), (np.uint16, (33, 65, 3))])
def test_png_round_trip(tmp_path, dtype, shape):
    from sdformerflow_amd.utils import png
    r = np.random.default_rng(3)
    img = r.integers(0, np.iinfo(dtype).max + 1, shape).astype(dtype)
    img.reshape(-1)[:2] = (0, np.iinfo(dtype).max)
    path = str(tmp_path / "a.png")
    png.write_png(path, img)
    back = png.read_png(path)
    assert back.dtype == dtype and np.array_equal(back, img)
    if dtype == np.uint16:                                      # big-endian samples in the file, as the format asks
        data = open(path, "rb").read()
        assert data[:8] == b"\x89PNG\r\n\x1a\n" and data[24] == 16 and data[25] == 2
    else:
        try:
            from PIL import Image
        except ImportError:
            return
        assert np.array_equal(np.asarray(Image.open(path).convert("RGB")), img)


def test_png_reader_serves_every_row_filter_and_refuses_the_rest(tmp_path):
    """8-bit files PIL writes use the adaptive filters; the reader must undo them (when PIL is importable)."""
    from sdformerflow_amd.utils import png
    with pytest.raises(ValueError):
        png.encode_png(np.zeros((4, 4), np.uint8))
    with pytest.raises(ValueError):
        png.encode_png(np.zeros((4, 4, 3), np.float32))
    with pytest.raises(ValueError):
        png.decode_png(b"not a png file at all")
    good = png.encode_png(np.zeros((2, 2, 3), np.uint8))
    with pytest.raises(ValueError, match="CRC"):
        png.decode_png(good[:20] + bytes([good[20] ^ 1]) + good[21:])
    try:
        from PIL import Image
    except ImportError:
        return
    y, x = np.mgrid[0:40, 0:50]
    img = np.stack([(3 * x + y) % 256, (x * y) % 256, (5 * y) % 256], -1).astype(np.uint8)          # smooth: sub / up / average / paeth win
    path = str(tmp_path / "pil.png")
    Image.fromarray(img).save(path, optimize=True)
    assert np.array_equal(png.read_png(path), img)


# -- ABI ---------------------------------------------------------------------------------------------------------------------------
def test_new_entry_points_are_declared_exported_and_bound(lib):
    from sdformerflow_amd import hip
    src = open(os.path.join(ROOT, "include", "sdformerflow_hip.h")).read()
    declared = re.findall(r"^(?:int|int64_t|void) (sdf_\w+)\(", src, flags=re.M)
    for name in NEW:
        assert name in declared and name in hip.SIGNATURES and hasattr(lib, name), name
    for table in (declared, list(hip.SIGNATURES)):                # behind their siblings, in the header and in the binding's table
        at = table.index("sdf_prepare_chunk_fwd")
        assert table[at + 1:at + 5] == list(NEW)
    assert lib.sdf_version() == 107
    for mirror, size in ((hip.FlowImageDesc, 56), (hip.FlowSubmissionDesc, 32), (hip.EventImageDesc, 72)):
        assert C.sizeof(mirror) == size, mirror
    for fn in (hip.flow_image, hip.flow_submission, hip.event_image, hip.event_counts, hip.event_counts_image):
        assert callable(fn)
    build = open(os.path.join(ROOT, "sdformerflow_amd", "csrc", "build.sh")).read()
    assert " flow_render " in build and "flow_render.res" not in build


def test_flow_image_argument_errors_are_reported_before_any_launch(lib):
    from sdformerflow_amd import hip

    def call(**kw):
        d = hip.FlowImageDesc()
        d.flow, d.out, d.workspace, d.workspace_bytes, d.B, d.H, d.W = 0x10000, 0x20000, 0x30000, 1 << 20, 2, 16, 24
        for k, v in kw.items():
            setattr(d, k, v)
        return lib.sdf_flow_image_fwd(C.byref(d), None)

    assert lib.sdf_flow_image_fwd(None, None) == E_NULL
    for f in ("flow", "out", "workspace"):
        assert call(**{f: None}) == E_NULL, f
    for kw in ({"B": 0}, {"H": 0}, {"W": -1}, {"B": 65536}, {"H": 1 << 15, "W": 1 << 15}, {"workspace_bytes": 15}):
        assert call(**kw) == E_SHAPE, kw
    assert call(H=0, flow=None) == E_SHAPE                      # the shape comes first, as in sdf_flow_metrics_fwd
    for kw in ({"flow": 0x10002}, {"mask": 0x40001}, {"workspace": 0x30002}):
        assert call(**kw) == E_ALIGN, kw
    assert lib.sdf_flow_image_workspace_bytes(3, 16, 24) == 24
    for B, H, W in ((0, 16, 24), (65536, 16, 24), (1, 0, 24), (1, 16, 0), (1, 1 << 15, 1 << 15)):
        assert lib.sdf_flow_image_workspace_bytes(B, H, W) == 0


def test_flow_submission_argument_errors_are_reported_before_any_launch(lib):
    from sdformerflow_amd import hip

    def call(**kw):
        d = hip.FlowSubmissionDesc()
        d.flow, d.out, d.B, d.H, d.W = 0x10000, 0x20000, 2, 16, 24
        for k, v in kw.items():
            setattr(d, k, v)
        return lib.sdf_flow_submission_fwd(C.byref(d), None)

    assert lib.sdf_flow_submission_fwd(None, None) == E_NULL
    assert call(flow=None) == E_NULL and call(out=None) == E_NULL
    for kw in ({"B": 0}, {"H": 0}, {"W": 0}, {"B": 65536}, {"H": 1 << 15, "W": 1 << 15}):
        assert call(**kw) == E_SHAPE, kw
    assert call(flow=0x10002) == E_ALIGN and call(out=0x20001) == E_ALIGN


def test_event_image_argument_errors_are_reported_before_any_launch(lib):
    from sdformerflow_amd import hip

    def call(**kw):
        d = hip.EventImageDesc()
        d.src, d.chunk_vis, d.bounds, d.out = 0x10000, 0x20000, 0x30000, 0x40000
        d.B, d.bins, d.Hs, d.Ws, d.crop_h, d.crop_w, d.crop_oy, d.crop_ox = 2, 10, 20, 30, 16, 24, 1, 3
        for k, v in kw.items():
            setattr(d, k, v)
        return lib.sdf_event_image_fwd(C.byref(d), None)

    assert lib.sdf_event_image_fwd(None, None) == E_NULL
    assert call(src=None) == E_NULL and call(chunk_vis=None) == E_NULL and call(chunk_vis=None, stage=1) == E_NULL
    assert call(stage=1, bounds=None) == E_NULL and call(stage=1, out=None) == E_NULL
    for kw in ({"mode": 2}, {"mode": -1}, {"stage": 2}, {"stage": -1}):
        assert call(**kw) == E_DTYPE, kw
    for kw in ({"B": 0}, {"B": 65536}, {"bins": 0}, {"Hs": 0}, {"Ws": 0}, {"crop_h": -1}, {"crop_h": 0}, {"crop_w": 0},
               {"crop_oy": -1}, {"crop_ox": -1}, {"crop_oy": 5}, {"crop_ox": 7}, {"crop_h": 21, "crop_oy": 0}, {"crop_w": 31, "crop_ox": 0},
               {"crop_h": 0, "crop_w": 0}, {"Hs": 1 << 15, "Ws": 1 << 15, "crop_h": 0, "crop_w": 0, "crop_oy": 0, "crop_ox": 0},
               {"Hs": 1 << 24, "Ws": 1 << 24, "bins": 1 << 10}):
        assert call(**kw) == E_SHAPE, kw
    for kw in ({"src": 0x10002}, {"chunk_vis": 0x20001}, {"bounds": 0x30002, "stage": 1}):
        assert call(**kw) == E_ALIGN, kw


# -- the Python surface ------------------------------------------------------------------------------------------------------------
def test_cpu_tensors_raise():
    from sdformerflow_amd import hip
    flow = torch.zeros(1, 2, 4, 6)
    for call in (lambda: hip.flow_image(flow), lambda: hip.flow_submission(flow), lambda: hip.event_image(torch.zeros(1, 10, 4, 6)),
                 lambda: hip.event_image(torch.zeros(1, 10, 2, 4, 6)), lambda: hip.event_counts_image(flow)):
        with pytest.raises(hip.SdfError, match="no CPU fallback"):
            call()


def test_store_without_a_directory_is_refused_before_any_forward():
    from sdformerflow_amd import harness

    class Model:
        def __call__(self, x):
            raise AssertionError("a forward was run")
    cfg = {"vis": {"store": True}, "loader": {}, "metrics": {}, "model": {}, "data": {}}
    touched = []
    samples = (touched.append(1) for _ in range(1))              # (not even the first sample is drawn)
    for fn in (harness.evaluate, harness.evaluate_mv):
        with pytest.raises(ValueError, match="store_dir"):
            fn(Model(), samples, cfg, device="cpu")
    assert not touched
    with pytest.raises(RuntimeError, match="renders_out"):
        harness.StreamEvaluator(Model(), cfg, device="cpu")


def test_visualization_surface(tmp_path):
    """The reference's constructor, directory names and signature; what is not built says so."""
    import inspect
    from sdformerflow_amd.utils.visualization import Visualization_DSEC
    vis = Visualization_DSEC({"vis": {"px": 400}}, eval_id=3, path_results=str(tmp_path) + "/")
    assert os.path.isdir(tmp_path / "results" / "eval_3") and vis.img_idx == 0 and vis.px == 400
    assert list(inspect.signature(vis.store).parameters) == ["events", "gtflow", "mask", "flow", "sequence", "flow_test", "frames",
                                                             "events_window", "masked_window_flow", "iwe_window", "ts", "idx"]
    with pytest.raises(NotImplementedError, match="live cv2 window"):
        vis.update(None, None, None, None)
    z = torch.zeros(1, 2, 4, 6)
    with pytest.raises(ValueError, match="pass None"):
        vis.store(z, z, None, z, "seq", frames=z)
    with pytest.raises(ValueError, match="store directory"):
        Visualization_DSEC({"vis": {}}).store(z, z, None, z, "seq")
