"""The --flow-* options of examples/refine_illusion.py, refine_genomes.py, evolve_illusion.py and scripts/train_bench.py, and the flow
objective they state (train.make_flow).  The choices are those of train.FLOW_DIRECTIONS, FLOW_REFERENCES and FLOW_PAIRINGS; --flow-score and --flow-max-norm state a train.FlowScore."""

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
    "max-norm": dict(type=float, default=0.3, help="--flow-score: vectors longer than this many pixels are no members (the fitness's own limit is 0.3)"),
}


def add_flow_arguments(ap, names=tuple(FLOW_ARGUMENTS), **own):
    """--flow-<name> for every name; own: {name: the add_argument keywords a script states itself, in place of those above}"""
    for name in names:
        ap.add_argument("--flow-" + name, **dict(FLOW_ARGUMENTS[name], **own.get(name, {})))


def flow_of(a, w, h, mask=None):
    """the FlowObjective of the command line (None under another objective); the term counts the pixels of `mask`"""
    from evolutionary_illusion_generator_amd import train
    if a.objective != "flow":
        return None
    score = train.FlowScore(max_norm=a.flow_max_norm) if getattr(a, "flow_score", False) else None
    return train.make_flow(a.flow_pairing, a.flow_radius, a.flow_eps, None if a.flow_direction is None else train.flow_direction(a.flow_direction, w, h), mask,
                           reference=a.flow_reference, score=score)
