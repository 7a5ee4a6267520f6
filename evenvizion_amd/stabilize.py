"""Command-line driver of the stabilised view, with the arguments of the reference's
evenvizion/examples/compare_evenvizion_with_original_video.py plus --mode, --placement, --scale, --trail, --comparison, --plate,
--surface, --blend and --steady:

    python -m evenvizion_amd.stabilize --path_to_homography_dict run1/video/dict_with_homography_matrix.json \
           --path_to_video video.mp4 --experiment_name run1 --comparison 1

writes into  <cwd>/<experiment_name>/<video stem>/visualize_camera_stabilization/ , produced on the MI355X by
evenvizion_amd.stabilization:

    --comparison 1   NNNNNN.png per frame, the reference's picture: the original frame beside the fixed plane, both 300 rows
                     high; in the plane earlier frames fade out behind the current one, which sits in its white rectangle
                     (--placement translate), and the plane sits in the red canvas border;
    --trail 1        NNNNNN.ppm per frame: that fixed-plane picture alone, at the canvas's own size, as binary P6;
    neither          NNNNNN.ppm per frame (one file for --mode mosaic): the canvas of the fixed coordinate system, geometry
                     only -- no dimming, no border;
    --plate 1        plate.ppm, the scene without its moving objects (the per-pixel median of up to --plate_frames frames spread
                     over the video, where at least --plate_min_cover of them cover the pixel), plate_count.png, how many frames
                     cover each pixel, and with --plate_masks 1 mask_NNNNNN.png per frame taken: white where that frame differs
                     from the plate by more than --plate_threshold gray levels.  With --plate_objects 1 also
                     moving_objects.json: per frame taken the connected components of its mask after an opening (--object_open R,
                     --object_connectivity 4 | 8, --object_min_area N, at most --object_max N per frame) with box, centre and area
                     on the plane and in the frame, linked into tracks by box overlap (evenvizion_amd.moving.moving_objects); with
                     --plate_masks 1 then labels_NNNNNN.png too: gray ((label - 1) mod 255) + 1, background 0.
    --surface cylinder | sphere
                     NNNNNN.ppm per frame (one file for --mode mosaic): the canvas of a fixed cylinder or sphere around the camera
                     of frame 1 instead of the fixed plane, for a camera that turns by more than the plane can hold (a pan beyond
                     90 degrees; evenvizion_amd.surface), and surface_report.json: the focal length (--focal F in pixels of the
                     resized frame, estimated from the matrices without it), the fit residual of the rotation model per pair, the
                     canvas geometry.  --scale applies; --placement does not.

    --mode mosaic --blend feather | seam
                     mosaic_blend.ppm instead of the last-frame-wins mosaic: every covering frame weighted by its distance to
                     its own border, rising over --feather PX pixels (feather), or per pixel the frame whose border is farthest
                     away (seam); with --exposure 1 the video is first read once more for the overlap sums, one gain per frame
                     and channel is solved from them (exposure_gains.json) and applied.  On the plane or with --surface.

    --steady 1       steady_NNNNNN.ppm per frame: the video itself, at its own size (times --scale), on a smoothed camera path
                     (evenvizion_amd.steady): every frame's corners follow the Gaussian mean of their neighbours' over
                     --steady_radius R frames on each side (--steady_sigma S, default R / 2), the picture is enlarged by
                     --steady_zoom Z (auto: the least zoom, up to 1.25, that keeps every picture inside its frame), and what a
                     frame still leaves uncovered is filled from the --steady_fill F frames before and after it, feathered over
                     --steady_feather PX pixels.  Always writes steady_report.json: the zoom, the jitter of the path before and
                     after, per frame the shares its own frame and its neighbours gave.  With --format jpeg steady_NNNNNN.jpg,
                     with mjpeg one steady.avi.  Not with --trail, --comparison, --plate, --surface or --blend.

    --format jpeg | mjpeg
                     the pictures leave the device compressed (evenvizion_amd.pictures, evh_jpeg_encode): jpeg writes NNNNNN.jpg in
                     place of NNNNNN.ppm, mjpeg one stabilized.avi (Motion-JPEG, --fps) a player opens; --quality 1..100,
                     --subsampling 420 | 444.  For the canvases per frame, --trail 1 and --surface; the one picture of --mode
                     mosaic, of --blend (mosaic_blend.jpg) and of --plate (plate.jpg) is encoded too -- a single picture is
                     written as .jpg under either format, --mode mosaic excepted, whose stabilized.avi has one frame.  Not with
                     --comparison.  The default, ppm, writes every file as before.

What is still missing from the reference's picture is its text ("Original", "EvenVizion").  The dimming is the arithmetic
include/evhip.h states for evh_trail_fixed_plane, not cv2.cvtColor compared byte for byte.
"""
import argparse
import os


def parser():
    ap = argparse.ArgumentParser(
        description="Stabilised view on MI355X (argument surface of compare_evenvizion_with_original_video.py).  By default "
                    "writes the fixed-plane canvas per frame as binary PPM, geometry only: no text, no border and no dimming "
                    "of earlier frames.  With --trail 1 earlier frames fade out and the frame is outlined; with "
                    "--comparison 1 the original is set beside that picture inside the canvas border, as PNG.  The "
                    "reference's text is never drawn.")
    ap.add_argument("--path_to_homography_dict", help="path to homography dict",
                    default="test_video_processing/test_video/dict_with_homography_matrix.json")
    ap.add_argument("--path_to_video", default="test_video/test_video.mp4")
    ap.add_argument("--experiment_name", help="folder to save experiment result", default="test_video_processing")
    ap.add_argument("--mode", choices=("history", "each", "mosaic"), default="history",
                    help="history: the canvas after every frame (the reference's picture); each: every frame alone; "
                         "mosaic: one canvas of all frames")
    ap.add_argument("--placement", choices=("warp", "translate"), default="translate",
                    help="translate: the reference's paste of the resized frame; warp: the projective warp of the full-size frame")
    ap.add_argument("--scale", type=float, default=1.0, help="warp only: canvas pixels per fixed-plane unit")
    ap.add_argument("--trail", type=int, choices=(0, 1), default=0,
                    help="1: earlier frames fade out behind the current one and (translate) the frame gets its white rectangle; "
                         "needs --mode history")
    ap.add_argument("--comparison", type=int, choices=(0, 1), default=0,
                    help="1: the reference's side-by-side picture (original | trail inside the canvas border) as NNNNNN.png")
    ap.add_argument("--plate", type=int, choices=(0, 1), default=0,
                    help="1: instead of the pictures per frame, plate.ppm (the median of the registered frames: the scene without "
                         "its moving objects) and plate_count.png (frames covering each pixel)")
    ap.add_argument("--plate_frames", type=int, default=64, help="plate: frames taken, spread over the video (1..255)")
    ap.add_argument("--plate_min_cover", type=int, default=1,
                    help="plate: a pixel fewer frames cover stays black (1..255)")
    ap.add_argument("--plate_masks", type=int, choices=(0, 1), default=0,
                    help="plate: 1 writes mask_NNNNNN.png per frame taken, white where the frame differs from the plate")
    ap.add_argument("--plate_threshold", type=int, default=16, help="plate: gray levels a mask pixel must differ by (0..255)")
    ap.add_argument("--plate_objects", type=int, choices=(0, 1), default=0,
                    help="plate: 1 labels the masks on the device and writes moving_objects.json (frames, objects, tracks, parameters)")
    ap.add_argument("--object_connectivity", type=int, choices=(4, 8), default=None, help="objects: 4 or 8 neighbours (default 8)")
    ap.add_argument("--object_open", type=int, default=None, help="objects: radius of the opening before labelling (0..3, default 1)")
    ap.add_argument("--object_min_area", type=int, default=None, help="objects: pixels an object must have (default 25)")
    ap.add_argument("--object_max", type=int, default=None, help="objects: table rows per frame (1..65535, default 256)")
    ap.add_argument("--surface", choices=("cylinder", "sphere"), default=None,
                    help="place the frames on a fixed cylinder or sphere instead of the fixed plane: no horizon, any pan angle; "
                         "also writes surface_report.json")
    ap.add_argument("--focal", type=float, default=None,
                    help="surface: focal length in pixels of the resized frame; estimated from the matrices when not given")
    ap.add_argument("--blend", choices=("feather", "seam", "bands"), default=None,
                    help="mosaic only: blend the covering frames (evenvizion_amd.blend) and write mosaic_blend.ppm; bands: "
                         "multi-band blending under the label mask of seam")
    ap.add_argument("--bands", type=int, default=None, help="blend bands: the pyramid has levels 0..N (0..8, default 5)")
    ap.add_argument("--feather", type=float, default=32.0, help="blend: pixels over which a frame's weight rises from its border")
    ap.add_argument("--exposure", type=int, choices=(0, 1), default=0,
                    help="blend: 1 solves one gain per frame and channel from the overlaps and writes exposure_gains.json")
    ap.add_argument("--steady", type=int, choices=(0, 1), default=0,
                    help="1: the video itself on a smoothed camera path, borders filled from neighbouring frames: "
                         "steady_NNNNNN.ppm (or .jpg, or steady.avi) and steady_report.json")
    ap.add_argument("--steady_radius", type=int, default=None, help="steady: frames on each side the path is averaged over (default 15)")
    ap.add_argument("--steady_sigma", type=float, default=None, help="steady: the Gaussian's sigma in frames (default radius / 2)")
    ap.add_argument("--steady_zoom", default=None, help="steady: a zoom factor, or auto (the default)")
    ap.add_argument("--steady_fill", type=int, default=None, help="steady: neighbours on each side that fill the borders (0..7, default 2)")
    ap.add_argument("--steady_feather", type=float, default=None, help="steady: pixels the fill is feathered over (0..255, default 8)")
    ap.add_argument("--format", choices=("ppm", "jpeg", "mjpeg"), default="ppm",
                    help="ppm: binary P6 per picture; jpeg: NNNNNN.jpg encoded on the device; mjpeg: stabilized.avi of those files")
    ap.add_argument("--quality", type=int, default=90, help="jpeg, mjpeg: 1..100, the usual scaling of the Annex K tables")
    ap.add_argument("--subsampling", choices=("420", "444"), default="420", help="jpeg, mjpeg: chroma sub-sampling")
    ap.add_argument("--fps", type=float, default=25.0, help="mjpeg: frames per second written into the AVI headers")
    return ap


def write_pictures(save_folder, args, files, name="%06d.jpg", video="stabilized.avi"):
    """--format jpeg | mjpeg: the (frame_no, bytes) of a generator of files as NNNNNN.jpg, or as the frames of stabilized.avi."""
    from .pictures import MjpegAviWriter, write_jpeg
    writer = None
    for frame_no, data in files:
        if args.format == "jpeg":
            write_jpeg(os.path.join(save_folder, name % frame_no), data)
            continue
        if writer is None:
            h, w = jpeg_size(data)
            writer = MjpegAviWriter(os.path.join(save_folder, video), w, h, args.fps)
        writer.write(data)
    if writer is not None:
        writer.close()


def jpeg_size(data):
    """(h, w) of a JPEG file, from its SOF0 segment (the segments are walked: a table may hold the marker's two bytes)."""
    at = 2
    while data[at + 1] != 0xC0:
        at += 2 + (data[at + 2] << 8 | data[at + 3])
    return data[at + 5] << 8 | data[at + 6], data[at + 7] << 8 | data[at + 8]


def main(argv=None):
    ap = parser()
    args = ap.parse_args(argv)
    if (args.trail or args.comparison) and args.mode != "history":
        ap.error("--trail and --comparison need --mode history")
    if args.plate and (args.trail or args.comparison):
        ap.error("--plate writes the plate only: not with --trail or --comparison")
    if not (1 <= args.plate_frames <= 255 and 1 <= args.plate_min_cover <= 255 and 0 <= args.plate_threshold <= 255):
        ap.error("--plate_frames and --plate_min_cover lie in 1..255, --plate_threshold in 0..255")
    given = [n for n in ("object_connectivity", "object_open", "object_min_area", "object_max") if getattr(args, n) is not None]
    if args.plate_objects and not args.plate:
        ap.error("--plate_objects needs --plate 1")
    if given and not args.plate_objects:
        ap.error("--%s needs --plate_objects 1" % given[0])
    objects = dict(connectivity=8 if args.object_connectivity is None else args.object_connectivity,
                   open_radius=1 if args.object_open is None else args.object_open,
                   min_area=25 if args.object_min_area is None else args.object_min_area,
                   max_objects=256 if args.object_max is None else args.object_max)
    if not (0 <= objects["open_radius"] <= 3 and objects["min_area"] >= 1 and 1 <= objects["max_objects"] <= 65535):
        ap.error("--object_open lies in 0..3, --object_min_area is at least 1, --object_max lies in 1..65535")
    if args.surface and (args.trail or args.comparison or args.plate):
        ap.error("--surface writes the canvases only: not with --trail, --comparison or --plate")
    if args.focal is not None and not args.surface:
        ap.error("--focal needs --surface")
    if args.focal is not None and not args.focal > 0:
        ap.error("--focal must be positive")
    if args.blend and (args.mode != "mosaic" or args.trail or args.comparison or args.plate):
        ap.error("--blend needs --mode mosaic, without --trail, --comparison or --plate")
    if not args.blend and (args.exposure or args.feather != 32.0):
        ap.error("--feather and --exposure need --blend")
    if not 0 <= args.feather <= 2047:
        ap.error("--feather lies in 0..2047 pixels")
    if args.blend != "bands" and args.bands is not None:
        ap.error("--bands needs --blend bands")
    if args.format == "ppm" and (args.quality != 90 or args.subsampling != "420" or args.fps != 25.0):
        ap.error("--quality, --subsampling and --fps need --format jpeg or mjpeg")
    if args.format != "ppm" and args.comparison:
        ap.error("--comparison writes PNG: not with --format jpeg or mjpeg")
    if not 1 <= args.quality <= 100 or not args.fps > 0:
        ap.error("--quality lies in 1..100, --fps is positive")
    coded = dict(quality=args.quality, subsampling=args.subsampling)
    steady = steady_arguments(ap, args)
    bands = 5 if args.bands is None else args.bands
    if not 0 <= bands <= 8:
        ap.error("--bands lies in 0..8")
    from .component import open_capture
    from .processing.utils import read_homography_dict, superposition_dict
    from .stabilization import comparison_frames, stabilized_frames, write_ppm
    cap, _, stem = open_capture(args.path_to_video)
    save_folder = os.path.join(os.getcwd(), args.experiment_name, stem, "visualize_camera_stabilization")
    os.makedirs(save_folder, exist_ok=True)
    homography_dict, resize_info = read_homography_dict(args.path_to_homography_dict)
    sup = superposition_dict(homography_dict)
    if args.steady:
        import json
        from .steady import steady_frames, steady_jpegs, steady_report
        report = {}
        if args.format != "ppm":
            write_pictures(save_folder, args, steady_jpegs(cap, sup, resize_info, scale=args.scale, report=report, **steady, **coded),
                           "steady_%06d.jpg", "steady.avi")
        else:
            for frame_no, picture in steady_frames(cap, sup, resize_info, scale=args.scale, report=report, **steady):
                write_ppm(os.path.join(save_folder, "steady_%06d.ppm" % frame_no), picture)
        with open(os.path.join(save_folder, "steady_report.json"), "w") as f:
            json.dump(steady_report(report), f, indent=1)
        return save_folder
    if args.blend:
        import json
        from .blend import blended_mosaic, exposure_pairs, exposure_stats, solve_gains, surface_pair_maps
        placement = "warp" if args.surface else args.placement
        gains = None
        if args.exposure:
            keys = [k for k in sup if k != "resize_info"]
            maps = None
            if args.surface:
                from .surface import surface_model
                model = surface_model(sup, resize_info, surface=args.surface, focal=args.focal, scale=args.scale)
                maps = surface_pair_maps(model, keys, exposure_pairs(len(keys)))
            pairs, stats = exposure_stats(cap, sup, resize_info, maps=maps)
            gains = solve_gains(pairs, stats, len(keys))
            with open(os.path.join(save_folder, "exposure_gains.json"), "w") as f:
                json.dump({"pairs": len(pairs), "pairs_used": int((stats[:, 0] >= 64).sum()),
                           "gains": {str(k): [float(v) for v in g] for k, g in zip(keys, gains)}}, f, indent=1)
            cap, _, _ = open_capture(args.path_to_video)          # the second pass starts from the first frame again
        picture = blended_mosaic(cap, sup, resize_info, blend=args.blend, feather_px=args.feather, gains=gains, placement=placement,
                                 scale=args.scale, surface=args.surface, focal=args.focal, bands=bands)
        if args.format == "ppm":
            write_ppm(os.path.join(save_folder, "mosaic_blend.ppm"), picture)
        else:
            from .pictures import encode_jpeg, write_jpeg
            write_jpeg(os.path.join(save_folder, "mosaic_blend.jpg"), encode_jpeg(picture, **coded)[0])
        return save_folder
    if args.surface:
        import json
        from .surface import surface_frames, surface_model, surface_report
        model = surface_model(sup, resize_info, surface=args.surface, focal=args.focal, scale=args.scale)
        with open(os.path.join(save_folder, "surface_report.json"), "w") as f:
            json.dump(surface_report(model), f, indent=1)
        if args.format != "ppm":
            from .surface import surface_jpegs
            write_pictures(save_folder, args, surface_jpegs(cap, sup, resize_info, surface=args.surface, focal=model.focal,
                                                            mode=args.mode, scale=args.scale, **coded))
            return save_folder
        for frame_no, picture in surface_frames(cap, sup, resize_info, surface=args.surface, focal=model.focal, mode=args.mode,
                                                scale=args.scale):
            write_ppm(os.path.join(save_folder, "%06d.ppm" % frame_no), picture)
        return save_folder
    if args.plate:
        from .matching_pictures import write_png
        from .stabilization import background_plate
        got = background_plate(cap, sup, resize_info, placement=args.placement, scale=args.scale, max_frames=args.plate_frames,
                               min_cover=args.plate_min_cover, masks=bool(args.plate_masks), threshold=args.plate_threshold)
        if args.format == "ppm":
            write_ppm(os.path.join(save_folder, "plate.ppm"), got.plate)
        else:
            from .pictures import encode_jpeg, write_jpeg
            write_jpeg(os.path.join(save_folder, "plate.jpg"), encode_jpeg(got.plate, **coded)[0])
        write_png(os.path.join(save_folder, "plate_count.png"), got.count, gray=True)
        for k, frame_no in enumerate(got.frame_nos if args.plate_masks else ()):
            write_png(os.path.join(save_folder, "mask_%06d.png" % frame_no), got.masks[k], gray=True)
        if args.plate_objects:
            write_moving_objects(save_folder, open_capture(args.path_to_video)[0], sup, resize_info, args, objects)
        return save_folder
    if args.comparison:
        from .matching_pictures import write_png
        for frame_no, picture in comparison_frames(cap, sup, resize_info, placement=args.placement, scale=args.scale):
            write_png(os.path.join(save_folder, "%06d.png" % frame_no), picture)
        return save_folder
    if args.format != "ppm":
        from .stabilization import stabilized_jpegs
        write_pictures(save_folder, args, stabilized_jpegs(cap, sup, resize_info, mode=args.mode, placement=args.placement,
                                                           scale=args.scale, trail=bool(args.trail), **coded))
        return save_folder
    for frame_no, picture in stabilized_frames(cap, sup, resize_info, mode=args.mode, placement=args.placement,
                                               scale=args.scale, trail=bool(args.trail)):
        write_ppm(os.path.join(save_folder, "%06d.ppm" % frame_no), picture)
    return save_folder


def steady_arguments(ap, args):
    """The refusals of --steady and its options -> the keyword arguments of steady.steady_frames."""
    given = [n for n in ("steady_radius", "steady_sigma", "steady_zoom", "steady_fill", "steady_feather") if getattr(args, n) is not None]
    if given and not args.steady:
        ap.error("--%s needs --steady 1" % given[0])
    if not args.steady:
        return None
    for flag in ("trail", "comparison", "plate", "surface", "blend"):
        if getattr(args, flag):
            ap.error("--steady writes the steady view only: not with --%s" % flag)
    zoom = "auto" if args.steady_zoom in (None, "auto") else None
    if zoom is None:
        try:
            zoom = float(args.steady_zoom)
        except ValueError:
            ap.error("--steady_zoom is a number or auto")
    got = dict(radius=15 if args.steady_radius is None else args.steady_radius, sigma=args.steady_sigma, zoom=zoom,
               fill=2 if args.steady_fill is None else args.steady_fill, feather_px=8.0 if args.steady_feather is None else args.steady_feather)
    from .steady import check_steady_arguments
    try:
        check_steady_arguments(got["radius"], got["sigma"], got["zoom"], 1.25, got["fill"], got["feather_px"], args.scale, 32, "auto")
    except ValueError as e:
        ap.error("--steady: %s" % e)
    return got


def write_moving_objects(save_folder, cap, sup, resize_info, args, objects):
    """moving_objects.json, and labels_NNNNNN.png with --plate_masks 1: the video is read once more, from its first frame."""
    import json

    import numpy as np

    from .matching_pictures import write_png
    from .moving import moving_objects
    params = dict(placement=args.placement, scale=args.scale, max_frames=args.plate_frames, min_cover=args.plate_min_cover,
                  threshold=args.plate_threshold, **objects)
    got = moving_objects(cap, sup, resize_info, labels=bool(args.plate_masks), **params)
    report = {"parameters": params, "origin": list(got["origin"]), "size": list(got["size"]), "frame_nos": got["frame_nos"],
              "frames": {str(k): v for k, v in got["frames"].items()}, "tracks": [[list(step) for step in t] for t in got["tracks"]]}
    with open(os.path.join(save_folder, "moving_objects.json"), "w") as f:
        json.dump(report, f, indent=1)
    for k, frame_no in enumerate(got["frame_nos"] if args.plate_masks else ()):
        sheet = got["labels"][k]
        write_png(os.path.join(save_folder, "labels_%06d.png" % frame_no), np.where(sheet > 0, (sheet - 1) % 255 + 1, 0).astype(np.uint8),
                  gray=True)


if __name__ == "__main__":
    main()
