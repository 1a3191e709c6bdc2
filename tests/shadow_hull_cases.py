"""Scenes for SHADOW HULL (mitransient_amd/csrc/mtr_shadow_hull.h): rooms of rectangles with one rectangular light in which a
shadow ray of the fused kernel is spared the walls' rectangle tests ("on"), and the smallest changes that switch that off.
test_shadow_hull.py classifies them on the CPU (tests/host_shadow_hull.cpp: classify_scene), test_gpu_fused_shadow_hull.py renders
them.  Every builder returns the scene dictionary; `film` and `integrator` update the Cornell box's."""


def _T():
    from mitransient_amd.transform import ScalarTransform4f
    return ScalarTransform4f


def cornell(film=None, **integrator):
    import mitransient_amd as mitr
    import mitransient_amd.mi as mi
    mi.set_variant("llvm_ad_rgb")
    d = mitr.cornell_box()
    d["sensor"]["film"].update(width=32, height=24, temporal_bins=64, start_opl=0.0, bin_width_opl=12.0 / 64)
    d["sensor"]["film"].update(film or {})
    d["integrator"].update(amd_mode="fused", max_depth=6)
    d["integrator"].update(integrator)
    return d


def _white():
    return {"type": "ref", "id": "white"}


def _light(at, axis=(1, 0, 0), deg=90.0):
    return {"type": "rectangle", "to_world": _T()().translate(list(at)).rotate(list(axis), deg).scale([0.23, 0.19, 0.19]), "bsdf": _white(),
            "emitter": {"type": "area", "radiance": {"type": "rgb", "value": [18.387, 13.9873, 6.75357]}}}


# ---- off: each is the Cornell box with one thing changed
def second_emitter(**kw):
    d = cornell(**kw)
    d["far-light"] = {"type": "rectangle", "to_world": _T()().translate([0.5, 0.5, -0.98]).scale([0.05, 0.05, 0.05]), "bsdf": _white(),
                      "emitter": {"type": "area", "radiance": {"type": "rgb", "value": [2.0, 2.0, 2.0]}}}
    return d


def light_in_the_ceiling(**kw):
    d = cornell(**kw)
    d["light"] = _light([0.0, 1.0, 0.01])
    return d


def light_touching_a_wall(**kw):
    d = cornell(**kw)
    d["light"] = _light([0.77, 0.99, 0.01])          # reaches x = 1.0, the green wall's plane
    return d


def partition(**kw):
    d = cornell(**kw)
    d["partition"] = {"type": "rectangle", "to_world": _T()().translate([0.3, -0.5, 0.0]).rotate([0, 1, 0], 90.0).scale([0.4, 0.5, 1.0]), "bsdf": _white()}
    return d


def cube_through_the_floor(**kw):
    d = cornell(**kw)
    d["large-box"]["to_world"] = _T()().translate([-0.33, -0.7, -0.28]).rotate([0, 1, 0], 18.25).scale([0.3, 0.61, 0.3])      # 0.31 below the floor
    return d


OFF = {"second-emitter": second_emitter, "light-in-the-ceiling": light_in_the_ceiling, "light-touching-a-wall": light_touching_a_wall,
       "partition": partition, "cube-through-the-floor": cube_through_the_floor}


# ---- on
def scaled(factor, **kw):
    """the whole room, camera and clip planes included, times `factor`; the film's bins cover the same paths"""
    d = cornell(**kw)
    S = _T()().scale([factor, factor, factor])
    for name, obj in d.items():
        if isinstance(obj, dict) and obj.get("type") in ("rectangle", "cube"):
            obj["to_world"] = S @ obj["to_world"]
    d["sensor"]["to_world"] = _T()().look_at(origin=[0, 0, 3.90 * factor], target=[0, 0, 0], up=[0, 1, 0])
    d["sensor"].update(near_clip=0.001 * factor, far_clip=100.0 * factor)
    film = d["sensor"]["film"]
    film.update(start_opl=film["start_opl"] * factor, bin_width_opl=film["bin_width_opl"] * factor)
    return d


def light_on_the_red_wall(**kw):
    d = cornell(**kw)
    d["light"] = _light([-0.99, 0.1, 0.05], axis=(0, 1, 0), deg=90.0)
    return d


def seven_rectangles_one_cube(**kw):
    """a panel across the open side, the camera inside: seven rectangles — six hull rectangles and the light — and one cube, the
    most a root of eight children holds: the fourth slab pair, its second half a box"""
    d = cornell(**kw)
    d.pop("large-box")
    d["front"] = {"type": "rectangle", "to_world": _T()().translate([0.0, 0.0, 1.5]).rotate([1, 0, 0], 180.0), "bsdf": _white()}
    d["sensor"]["to_world"] = _T()().look_at(origin=[0, 0, 1.2], target=[0, -0.2, 0], up=[0, 1, 0])
    return d


def looking_at_the_light(**kw):
    """a film cropped to the pixels that see the light: camera rays end on E, the first shadow rays start there"""
    film = dict(width=64, height=64, crop_width=12, crop_height=4, crop_offset_x=26, crop_offset_y=7)
    film.update(kw.pop("film", None) or {})
    return cornell(film=film, **kw)


ON = {"cornell": cornell, "scaled-100": lambda **kw: scaled(100.0, **kw), "scaled-0.01": lambda **kw: scaled(0.01, **kw),
      "light-on-the-red-wall": light_on_the_red_wall, "seven-rectangles-one-cube": seven_rectangles_one_cube, "looking-at-the-light": looking_at_the_light}
HULL_RECTANGLES = {"cornell": 5, "scaled-100": 5, "scaled-0.01": 5, "light-on-the-red-wall": 5, "seven-rectangles-one-cube": 6, "looking-at-the-light": 5}
