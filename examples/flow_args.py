"""The --flow-* options of examples/refine_illusion.py, refine_genomes.py, evolve_illusion.py and scripts/train_bench.py, and the flow
objective they state (train.make_flow).  The choices are those of train.FLOW_DIRECTIONS, FLOW_REFERENCES and FLOW_PAIRINGS; --flow-score, --flow-score-structure and --flow-max-norm state a train.FlowScore, BandsScore or FreeScore; --flow-members, --flow-corner-quality and
--flow-corner-distance a train.CornerMembers."""

SCORE_STRUCTURES = {"bands": 0, "circles": 1, "free": 2}   # --flow-score-structure -> the fitness's number of the structure


FLOW_ARGUMENTS = {
    "direction": dict(default=None, choices=["tangent", "radial", "horizontal", "vertical"],
                      help="objective flow: climb the displacement along this field (default: its mean square)"),
    "radius": dict(type=int, default=7, help="objective flow: the window is 2 R + 1 pixels wide"),
    "eps": dict(type=float, default=1e-2, help="objective flow: the regulariser of the 2x2 systems"),
    "reference": dict(default="constant", choices=["constant", "moving"],
                      help="objective flow: moving also follows how the term moves with the still as its reference frame (constant: the input path alone)"),
    "pairing": dict(default="frame", choices=["frame", "prediction"],
                    help="objective flow: frame pairs the still with the extended predictions (the single-image fitness path), prediction pairs consecutive "
                         "predictions, as the population fitness printed here does; prediction takes --flow-reference constant only"),
    "score": dict(action="store_true", help="objective flow: climb the fitness's own Circles score of the dense field (train.FlowScore) in place of the "
                                             "displacement; it takes no --flow-direction"),
    "score-structure": dict(default="circles", choices=["circles", "bands", "free", "auto"],
                            help="--flow-score: the structure whose score is climbed: circles (train.FlowScore), bands (train.BandsScore), free (train.FreeScore), "
                                 "or auto, the script's own --structure"),
    "max-norm": dict(type=float, default=None, help="--flow-score: vectors longer than this many pixels are no members (default: the fitness's own limit for the "
                                                    "chosen structure, 0.3 circles, 0.15 bands, 0.4 free)"),
    "members": dict(default="all", choices=["all", "corners"],
                    help="--flow-score: the pixels that can be members of the score: all the mask counts, or corners, the points goodFeaturesToTrack picks on "
                         "every term's own reference, as the fitness does (train.CornerMembers)"),
    "corner-quality": dict(type=float, default=0.3, help="--flow-members corners: goodFeaturesToTrack's qualityLevel (the fitness's: 0.3)"),
    "corner-distance": dict(type=float, default=7.0, help="--flow-members corners: goodFeaturesToTrack's minDistance in pixels (the fitness's: 7)"),
    "levels": dict(type=int, default=1, help="objective flow: pyramid levels of the solve the gradient runs through (1 .. 6; 1 with --flow-iters 1 is the single step)"),
    "iters": dict(type=int, default=1, help="objective flow: window iterations per pyramid level (1 .. 32)"),
}


def add_flow_arguments(ap, names=tuple(FLOW_ARGUMENTS), **own):
    """--flow-<name> for every name; own: {name: the add_argument keywords a script states itself, in place of those above}"""
    for name in names:
        ap.add_argument("--flow-" + name, **dict(FLOW_ARGUMENTS[name], **own.get(name, {})))


def add_flow_target_argument(ap):
    """--flow-target of the scripts that train on videos with a known flow (examples/train_prednet.py, scripts/train_bench.py); a still
    has no truth, so the refinement scripts do not take it"""
    ap.add_argument("--flow-target", default="none", choices=["none", "truth"],
                    help="objective flow: truth makes every term the squared endpoint error of the solved field against the exact flow of the video "
                         "(train.MovingTextures' own, so it needs --data textures) in place of the mean squared displacement")


def check_flow_target(ap, a):
    """--flow-target truth without --data textures is an argparse error: no other source states its flow"""
    if a.flow_target == "truth" and getattr(a, "data", None) != "textures":
        ap.error("--flow-target truth needs --data textures: no other source states the flow of its frames")


def add_flow_joint_arguments(ap):
    """--frame-weight and --flow-valid of the scripts that train on videos (examples/train_prednet.py, scripts/train_bench.py): the joint
    objective and the valid pixels of ``forward_backward(frame_weight=, flow_valid=)``"""
    ap.add_argument("--frame-weight", type=float, default=None, metavar="MU",
                    help="objective flow: the loss is the flow objective's plus MU times the squared error of the predictions, in one backward pass")
    ap.add_argument("--flow-valid", default="none", choices=["none", "visible"],
                    help="--flow-target truth: visible counts a pixel only where its surface can be seen in the next frame (train.MovingTextures' "
                         "validity planes: inside the image and not covered by the second layer)")


def check_flow_joint(ap, a):
    """--frame-weight without --objective flow and --flow-valid visible without --data textures --flow-target truth are argparse errors"""
    if a.frame_weight is not None and getattr(a, "objective", None) != "flow":
        ap.error("--frame-weight is a mode of --objective flow")
    if a.flow_valid == "visible" and (getattr(a, "data", None) != "textures" or getattr(a, "flow_target", "none") != "truth"):
        ap.error("--flow-valid visible needs --data textures --flow-target truth: the planes state where the video's own flow can be recovered")
    if a.frame_weight is not None:
        from evolutionary_illusion_generator_amd.train import check_frame_weight
        try:
            check_frame_weight("flow", a.frame_weight)
        except ValueError as e:
            ap.error(str(e))


def score_of(a):
    """the score of the command line: None without --flow-score; else the class of --flow-score-structure (auto: of a.structure), with
    --flow-max-norm where it is given"""
    from evolutionary_illusion_generator_amd import train
    if not getattr(a, "flow_score", False):
        return None
    which = getattr(a, "flow_score_structure", "circles")
    if which == "auto":
        if getattr(a, "structure", None) is None:
            raise ValueError("--flow-score-structure auto needs a --structure")
        structure = int(a.structure)
    else:
        structure = SCORE_STRUCTURES[which]
    max_norm = getattr(a, "flow_max_norm", None)
    return train.structure_score(structure, **({} if max_norm is None else {"max_norm": max_norm}))


def members_of(a):
    """the members of the command line: None under --flow-members all; else a train.CornerMembers of --flow-corner-quality and
    --flow-corner-distance.  ValueError: corners without --flow-score"""
    from evolutionary_illusion_generator_amd import train
    if getattr(a, "flow_members", "all") != "corners":
        return None
    if not getattr(a, "flow_score", False):
        raise ValueError("--flow-members corners needs --flow-score: the displacement modes have no members")
    return train.CornerMembers(quality_level=getattr(a, "flow_corner_quality", 0.3), min_distance=getattr(a, "flow_corner_distance", 7.0))


def flow_of(a, w, h, mask=None):
    """the FlowObjective of the command line (None under another objective); the term counts the pixels of `mask`"""
    from evolutionary_illusion_generator_amd import train
    if a.objective != "flow":
        return None
    score = score_of(a)
    return train.make_flow(a.flow_pairing, a.flow_radius, a.flow_eps, None if a.flow_direction is None else train.flow_direction(a.flow_direction, w, h), mask,
                           reference=a.flow_reference, score=score, members=members_of(a), levels=a.flow_levels, iters=a.flow_iters)


def dense_fitness_of(a, structure, mask=None):
    """the fitness.DenseFitness of the command line under --fitness dense (None under corners): the window of --flow-radius and --flow-eps,
    the score of --flow-score where it is given (it must be `structure`'s: ValueError) and the structure's defaults otherwise, the
    pixels of `mask`, the solve of --dense-levels and --dense-iters, the members of --dense-members (corners: train.CornerMembers with
    --dense-corner-quality and --dense-corner-distance), the images of --dense-frames (float: PredNet's float predictions in place of the emitted bytes).  With --refine --objective flow --flow-score --flow-pairing prediction selection and refinement then use one score
    with the same settings."""
    from evolutionary_illusion_generator_amd import fitness
    if getattr(a, "fitness", "corners") != "dense":
        return None
    members = None
    if getattr(a, "dense_members", "all") == "corners":   # --dense-members corners: the sparse fitness's own corners, CornerMembers' defaults unless said otherwise
        from evolutionary_illusion_generator_amd import train
        kw = {k: v for k, v in (("quality_level", getattr(a, "dense_corner_quality", None)), ("min_distance", getattr(a, "dense_corner_distance", None))) if v is not None}
        members = train.CornerMembers(**kw)
    return fitness.DenseFitness(score_of(a), radius=a.flow_radius, eps=a.flow_eps, mask=mask, levels=getattr(a, "dense_levels", 1),
                                iters=getattr(a, "dense_iters", 1), members=members, frames=getattr(a, "dense_frames", "byte")).resolved(structure)
