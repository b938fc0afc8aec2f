"""What tests read out of a launch plan (nbc_describe_plan): its lines as dictionaries, and which op must have produced the
tensor every op reads, derived from the networks' topology.  tests/test_plan_abi.py checks the planner's buffers against the
map; tests/test_gpu_bf16_operands.py takes a kernel's stored operands by it."""
from neuralbarkcalculator_amd import topology


def parse(text):
    ops, bufs, identity = [], [], None
    for line in text.splitlines():
        f = line.split()
        if f[0] == "op":
            o = {"name": f[1], "kernel": f[2], "cat": []}
            for key, v in (x.split("=") for x in f[3:]):
                if key == "cat":
                    o["cat"].append(int(v))
                else:
                    o[key] = v if key == "ds" else int(v)
            ops.append(o)
        else:
            assert f[0] == "buf" and int(f[1]) == len(bufs)
            bufs.append(int(f[2]))
            if f[3:] == ["identity"]:
                assert identity is None, "one identity buffer per plan"
                identity = int(f[1])
    return ops, bufs, identity


def expected_reads(arch, bn, names, fused):
    """{(op, field): the op whose output that read must find}, from the networks' topology (the op names carry it).  fused:
    the conv3 of a pair reads the downsample's input (as x2) instead of the identity, and the downsample reads nothing."""
    units = {u.name: u for u in topology.conv_units(arch)}
    image = bn == "image"

    def out_of(unit):                                       # the op that leaves `unit`'s tensor as its readers want it
        return units[unit].bn + ".apply" if image and units[unit].bn else unit

    want, stream, block_in, have = {}, None, None, set(names)
    for name in names:
        u = units.get(name)
        if image and name.endswith((".stats", ".apply")):
            unit = next(x.name for x in units.values() if x.bn == name[:-6])
            want[(name, "in")] = unit                        # the raw convolution
            if name.endswith(".apply") and units[unit].residual:
                blk = unit[:-len(".conv3")]
                want[(name, "res")] = out_of(blk + ".downsample.0") if blk + ".downsample.0" in have else block_in
        elif name == "ingest":
            stream = name
        elif name in ("backbone.conv1", "backbone.maxpool", "backbone.model._conv_stem", "backbone.model._conv_head"):
            want[(name, "in")] = stream
            stream = out_of(name) if u else name
        elif name.endswith(".swish"):
            want[(name, "in")] = stream
            stream = name
        elif name.endswith(".conv1") and ".layer" in name:
            block_in = stream
            want[(name, "in")] = stream
        elif name.endswith(".conv2") and ".layer" in name:
            want[(name, "in")] = out_of(name[:-1] + "1")
        elif name.endswith(".downsample.0"):
            if not (fused and name in fused):
                want[(name, "in")] = block_in
        elif name.endswith(".conv3") and ".layer" in name:
            blk = name[:-len(".conv3")]
            want[(name, "in")] = out_of(blk + ".conv2")
            if fused and name in fused.values():
                want[(name, "x2")] = block_in
            elif not image:
                want[(name, "res")] = blk + ".downsample.0" if blk + ".downsample.0" in have else block_in
            stream = out_of(name)
        elif name.endswith("._expand_conv"):
            block_in = stream
            want[(name, "in")] = stream
        elif name.endswith("._depthwise_conv"):
            blk = name[:-len("._depthwise_conv")]
            if blk + "._expand_conv" not in have:
                block_in = stream
            want[(name, "in")] = blk + "._expand_conv" if blk + "._expand_conv" in have else stream
        elif name.endswith("._se_expand"):
            want[(name, "in")] = name[:-len("._se_expand")] + "._depthwise_conv"     # its squeeze partials
        elif name.endswith(".gated_weights"):
            want[(name, "gate")] = name[:-len("._project_conv.gated_weights")] + "._se_expand"
        elif name.endswith("._project_conv"):
            want[(name, "in")] = name[:-len("._project_conv")] + "._depthwise_conv"
            want[(name, "gate")] = name + ".gated_weights"
            if u.residual:
                want[(name, "res")] = block_in
            stream = name
        elif name in ("classifier.0", "classifier.0.convs.4") or name.startswith("classifier.0.convs."):
            want[(name, "in")] = stream                     # the head reads the trunk
        elif name == "classifier.0.concat":
            for i, b in enumerate(["classifier.0.convs.%d.0" % k for k in range(4)] + ["classifier.0.convs.4"]):
                want[(name, "cat%d" % i)] = b
        elif name == "classifier.0.project.0":
            want[(name, "in")] = "classifier.0.concat"
        elif name == "classifier.1":
            want[(name, "in")] = "classifier.0.project.0"
        elif name == "classifier.4":
            want[(name, "in")] = "classifier.1" if "classifier.1" in units else out_of("classifier.0")
        else:
            assert name == "upsample_argmax", name
    return want
