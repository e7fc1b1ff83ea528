"""CPU check of device_fusion.integrate_depth_by_arguments: which of the four depth-mode entry points each combination of
(warp, colour_image, pixel_weight / carve) reaches, with which arguments, and which unpack_* function comes back."""
import pytest

MODEL = ("tsdf", "weight", "depth", "code", "camera", "offset", "twist")
GEN = (0.005, 15.0, 0.5, 6.0)  # voxel_size, narrow_band_width_voxels, w, max_weight

# (keyword arguments, entry point, unpacker, the arguments the entry point must receive)
CASES = [
    (dict(), "integrate_depth", "unpack_record", MODEL + GEN),
    (dict(colour="volume"), "integrate_depth", "unpack_record", MODEL + GEN),
    (dict(pixel_weight="pw"), "integrate_depth_weighted", "unpack_weighted_record", MODEL + GEN + ("pw", False)),
    (dict(carve=True), "integrate_depth_weighted", "unpack_weighted_record", MODEL + GEN + (None, True)),
    (dict(colour="volume", colour_image="image", colour_band=0.25), "integrate_depth_colour", "unpack_colour_record",
     MODEL[:2] + ("volume",) + MODEL[2:] + ("image",) + GEN + (None, False, 0.25)),
    (dict(colour="volume", colour_image="image", pixel_weight="pw", carve=True), "integrate_depth_colour",
     "unpack_colour_record", MODEL[:2] + ("volume",) + MODEL[2:] + ("image",) + GEN + ("pw", True, 1.0)),
    (dict(warp="psi"), "integrate_depth_warped", "unpack_warped_record",
     MODEL + ("psi",) + GEN + (None, False, None, None, 1.0)),
    (dict(warp="psi", colour="volume"), "integrate_depth_warped", "unpack_warped_record",
     MODEL + ("psi",) + GEN + (None, False, None, None, 1.0)),
    (dict(warp="psi", pixel_weight="pw", carve=True, colour="volume", colour_image="image", colour_band=0.5),
     "integrate_depth_warped", "unpack_warped_record", MODEL + ("psi",) + GEN + ("pw", True, "volume", "image", 0.5)),
]


@pytest.mark.parametrize("kw,entry,unpacker,want", CASES, ids=[c[1][16:] + "-" + "-".join(sorted(c[0])) for c in CASES])
def test_the_arguments_pick_the_entry_point(monkeypatch, kw, entry, unpacker, want):
    from levelsetfusion_python_amd import device_fusion
    calls = []
    for name in ("integrate_depth", "integrate_depth_weighted", "integrate_depth_colour", "integrate_depth_warped"):
        def fake(*args, _name=name, **kwargs):
            calls.append((_name, args, kwargs))
            return "record of " + _name
        monkeypatch.setattr(device_fusion, name, fake)
    record, unpack = device_fusion.integrate_depth_by_arguments(*MODEL, *GEN, **kw)
    assert calls == [(entry, want, {})]
    assert record == "record of " + entry and unpack is getattr(device_fusion, unpacker)
