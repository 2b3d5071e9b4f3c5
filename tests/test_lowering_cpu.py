"""export.py lowers graph.py's node list to the op table; nothing else states the topology. These tests read the table
back against the node list, structurally (no arithmetic): an offset, a source slice, a residual or an upsample flag that
disagrees with the graph still yields a loadable engine file, so it is caught here."""
import pytest

CASES = {"A": dict(), "A_lite_p2": dict(lite_p2=True), "A_base16": dict(base_channels=16),
         "B": dict(variant="B"), "B_base16": dict(variant="B", base_channels=16)}


@pytest.fixture(scope="module", params=list(CASES))
def built(request, pkg):
    from unina_yolo_dla_amd import export
    g = pkg.graph.Graph(in_h=64, in_w=64, **CASES[request.param])
    b = export.EngineBuilder(pkg.synth.make_state_dict(7, g), g)
    return b, b.g                                     # b.g: the graph the table was lowered from (widened for base 16)


def _carriers(b):
    """conv module path -> [(op, seg)] over the conv and stem ops."""
    from unina_yolo_dla_amd import export
    out = {}
    for op in b.ops:
        if op.kind in (export.OP_CONV, export.OP_STEM):
            for sg in op.segs:
                out.setdefault(sg.module, []).append((op, sg))
    return out


def _stored_at(b, g, i):
    """(buffer, channel offset, channels) where the op table stores node i's tensor, found from the ops alone."""
    from unina_yolo_dla_amd import export
    if i < 0:
        (images,) = [j for j, buf in enumerate(b.buffers) if buf[5] & export.BUF_INPUT]
        return images, 0, 3
    n = g.nodes[i]
    if n.kind in ("conv", "convout"):
        ((op, sg),) = _carriers(b)[n.name]
        return sg.dst.buf, sg.dst.coff, sg.n_count
    if n.kind == "add":                                # stored by the conv it closes (srcs = [shortcut, conv])
        return _stored_at(b, g, n.srcs[1])
    if n.kind == "up2":                                # stored by its producer, upsampled
        return _stored_at(b, g, n.srcs[0])
    if n.kind == "pool5":                              # the one pool op stores the whole chain behind the pools' input
        chain, x = [n.idx], n.srcs[0]
        while g.nodes[x].kind == "pool5":
            chain.append(x)
            x = g.nodes[x].srcs[0]
        xb, xoff, xc = _stored_at(b, g, x)
        (pool,) = [op for op in b.ops if op.kind == export.OP_SPPF_POOL and op.src_buf == xb]
        (sg,) = pool.segs
        assert sg.dst.buf == xb and sg.src_coff == xoff and pool.cin == xc and sg.n_count % xc == 0
        assert len(chain) <= sg.n_count // xc
        return xb, sg.dst.coff + (len(chain) - 1) * xc, xc
    assert n.kind == "cat"
    (buf,) = [j for j, rec in enumerate(b.buffers) if rec[0] == n.name]
    return buf, 0, n.c


def test_every_conv_node_is_one_seg_with_the_nodes_geometry(built):
    b, g = built
    carriers = _carriers(b)
    assert sorted(carriers) == sorted(n.name for n in g.convs())
    for n in g.convs():
        assert len(carriers[n.name]) == 1, n.name
        op, sg = carriers[n.name][0]
        _, ih, iw = g._shape(n.srcs[0])
        assert (op.cin, op.k, op.s, op.in_hw, op.out_hw, sg.n_count) == (n.cin, n.k, n.s, (ih, iw), (n.h, n.w), n.c), n.name
        assert bool(op.relu) == sg.bn == (n.kind == "conv"), n.name          # ConvBlock: BN + ReLU; convout: neither
        # it reads exactly where its producer's tensor is stored (a concat member's other users read the slice)
        assert (op.src_buf, sg.src_coff, op.cin) == _stored_at(b, g, n.srcs[0]), n.name
        assert b.buffers[op.src_buf][1:3] == [ih, iw], n.name


def test_every_concat_is_one_buffer_tiled_by_its_members_in_order(built):
    b, g = built
    cats = [n for n in g.nodes if n.kind == "cat"]
    assert len(cats) == (14 if g.variant == "B" else 12) - (1 if g.lite_p2 else 0)
    for n in cats:
        assert [rec[0] for rec in b.buffers].count(n.name) == 1, n.name
        buf, _, _ = _stored_at(b, g, n.idx)
        assert b.buffers[buf][1:4] == [n.h, n.w, n.c], n.name
        off = 0
        for m in n.srcs:
            assert _stored_at(b, g, m) == (buf, off, g.nodes[m].c), (n.name, g.nodes[m].name)
            off += g.nodes[m].c
        assert off == n.c == b.buffers[buf][3], n.name                       # no gap, no overlap, nothing left over


def test_every_add_is_the_res_of_the_op_carrying_its_conv(built):
    b, g = built
    carriers = _carriers(b)
    adds = [n for n in g.nodes if n.kind == "add"]
    assert adds
    closing = set()
    for n in adds:
        shortcut, conv = n.srcs
        op, sg = carriers[g.nodes[conv].name][0]
        assert op.res is not None and len(op.segs) == 1, n.name
        assert (op.res.buf, op.res.coff, op.res.c) == _stored_at(b, g, shortcut), n.name
        assert (sg.dst.buf, sg.dst.coff) != (op.res.buf, op.res.coff), n.name
        closing.add(id(op))
    assert all((op.res is not None) == (id(op) in closing) for op in b.ops)  # and no residual without an add


def test_every_up2_is_a_flag_on_its_producers_seg(built):
    from unina_yolo_dla_amd import export
    b, g = built
    carriers = _carriers(b)
    ups = [n for n in g.nodes if n.kind == "up2"]
    assert len(ups) == (3 if g.variant == "B" else 2)
    flagged = set()
    for n in ups:
        op, sg = carriers[g.nodes[n.srcs[0]].name][0]
        assert sg.flags & export.SEG_UP2, n.name
        assert b.buffers[sg.dst.buf][1:3] == [n.h, n.w] == [2 * op.out_hw[0], 2 * op.out_hw[1]], n.name
        flagged.add(id(sg))
    assert all(bool(sg.flags & export.SEG_UP2) == (id(sg) in flagged) for op in b.ops for sg in op.segs)
    assert not any(op.kind == export.OP_UPSAMPLE for op in b.ops)            # folded, never an op of its own


def test_the_six_outputs_are_written_exactly_once(built, pkg):
    from unina_yolo_dla_amd import export
    b, g = built
    outs = [j for j, rec in enumerate(b.buffers) if rec[5] & export.BUF_OUTPUT]
    assert [b.buffers[j][0] for j in outs] == list(pkg.graph.OUTPUT_NAMES)
    for j, i in zip(outs, g.outputs):
        n = g.nodes[i]
        writers = [(op, sg) for op in b.ops for sg in op.segs if sg.dst.buf == j]
        assert len(writers) == 1, n.name
        op, sg = writers[0]
        assert sg.module == n.name and (sg.dst.coff, sg.n_count) == (0, n.c) and sg.flags == export.SEG_PLANAR_F32
        assert b.buffers[j][1:5] == [n.h, n.w, n.c, export.BUF_F32_PLANAR] and not op.relu and not sg.bn
        assert not any(op.src_buf == j for op in b.ops)
    # the planar store goes to the outputs and nowhere else
    assert all(bool(sg.flags & export.SEG_PLANAR_F32) == (sg.dst.buf in outs) for op in b.ops for sg in op.segs)


def test_blocks_partition_the_compute_nodes(built):
    """graph.Block records are the units of lowering: every conv / convout / add / pool5 node belongs to exactly one."""
    b, g = built
    member = [i for blk in g.blocks for i in blk.nodes]
    assert len(member) == len(set(member))
    loose = {n.kind for n in g.nodes if n.idx not in set(member)}
    assert loose <= {"cat", "up2"}, loose                                    # network-level concats and upsamples only
    assert [blk.label for blk in g.blocks if blk.label] == ["p2_fused", "p3_out", "p4_out"]
