"""Proposal-list text files: the input format of the reference's trainer and tester
(/root/reference/ops/io.py:7-59; written by gen_proposal_list.py, read by ssn_dataset.py:158).

Two flavours share one layout::

    # <index>
    <video id or frame folder>
    <a>                 normalised list: a = 1           processed list: a = frame count
    <b>                 normalised list: b = 1           processed list: b = 1          (n_frame = int(a * b))
    <number of ground-truth instances>
    <label> <start> <end>                                   one line each
    <number of proposals>
    <label> <best IoU> <overlap with itself> <start> <end>  one line each

``load_proposal_file`` returns the reference's tuples ``(vid, n_frame, gt_boxes, pr_boxes)`` with the box fields
still as strings; ``process_proposal_list`` converts normalised positions to frame indices.
"""
import fnmatch
import glob
import os


def _records(lines):
    """Split the file into per-video records: runs of lines between '#' header lines."""
    rec = []
    for line in lines:
        if line.startswith('#'):
            if rec:
                yield rec
            rec = []
        else:
            rec.append(line.strip())
    if rec:
        yield rec


def load_proposal_file(filename):
    """-> [(vid, n_frame, [[label, start, end], ...], [[label, iou, overlap_self, start, end], ...]), ...]"""
    with open(filename) as f:
        lines = list(f)
    out = []
    for info in _records(lines):
        vid = info[0]
        n_frame = int(float(info[1]) * float(info[2]))
        n_gt = int(info[3])
        gt_boxes = [x.split() for x in info[4:4 + n_gt]]
        n_pr = int(info[4 + n_gt])
        pr_boxes = [x.split() for x in info[5 + n_gt:5 + n_gt + n_pr]]
        out.append((vid, n_frame, gt_boxes, pr_boxes))
    return out


def format_window_list_record(path, frame_cnt, duration, gt, named_proposals):
    """One video's record of a proposal list written from spans in SECONDS: the text of the reference's
    ``dump_window_list`` (/root/reference/ops/io.py:95-134), with the frame count given instead of counted from a frame
    folder.  gt: ``[(label, (start, end)), ...]`` (label + 1 is written), named_proposals: the tuples of
    ``tag_proposals.name_proposals``; positions become frame numbers at frame_cnt / duration frames per second."""
    real_fps = float(frame_cnt) / float(duration)
    gts = ["{} {} {}".format(g[0] + 1, int(g[1][0] * real_fps), int(g[1][1] * real_fps)) for g in gt]
    prs = ["{} {:.04f} {:.04f} {} {}".format(p[0], p[1], p[2], int(p[3] * real_fps), int(p[4] * real_fps))
           for p in named_proposals]
    return "{}\n{}\n{}\n{}\n{}{}\n{}\n".format(path, frame_cnt, 1, len(gts), "\n".join(gts) + ("\n" if gts else ""),
                                               len(prs), "\n".join(prs))


def format_window_list_rows(path, frame_cnt, gt_labels, gt_frames, labels, iou, overlap_self, frames):
    """The text of ``format_window_list_record`` from the arrays of ``proposal_lists.ProposalListBuilder.build`` (one
    video: ``result.rows(i)``), whose positions are frame numbers already: gt_labels [n] (label + 1, as written),
    gt_frames [n, 2], labels / iou / overlap_self [K], frames [K, 2]."""
    # (%-formatting of whole columns: the same digits as the reference's '{:.04f}'.format, cheaper than a format call per field)
    gts = list(map("%d %d %d".__mod__, zip(gt_labels.tolist(), gt_frames[:, 0].tolist(), gt_frames[:, 1].tolist())))
    prs = list(map("%d %.4f %.4f %d %d".__mod__, zip(labels.tolist(), iou.tolist(), overlap_self.tolist(),
                                                     frames[:, 0].tolist(), frames[:, 1].tolist())))
    return "{}\n{}\n{}\n{}\n{}{}\n{}\n".format(path, frame_cnt, 1, len(gts), "\n".join(gts) + ("\n" if gts else ""),
                                               len(prs), "\n".join(prs))


def parse_directory(path, key_func=lambda x: x[-11:], rgb_prefix='img_', flow_x_prefix='flow_x_', flow_y_prefix='flow_y_'):
    """``frame_dict[key_func(folder)] = (folder, RGB frames, flow frames)`` for every folder under ``path``, counted by file
    name prefix (/root/reference/ops/io.py:64-93); a folder with different numbers of x and y flow images is an error.
    Folders are taken in alphabetical order (of two with one key the later wins)."""
    frame_dict = {}
    for folder in sorted(glob.glob(os.path.join(path, '*'))):
        names = os.listdir(folder)
        rgb, x_cnt, y_cnt = (len(fnmatch.filter(names, prefix + '*')) for prefix in (rgb_prefix, flow_x_prefix, flow_y_prefix))
        if x_cnt != y_cnt:
            raise ValueError('x and y direction have different number of flow images. video: ' + folder)
        frame_dict[key_func(folder)] = (folder, rgb, x_cnt)
    return frame_dict


def write_proposal_file(filename, records):
    """The records of ``format_window_list_record`` under '# <index>' headers counted from 1, as the reference's
    proposal scripts write them (gen_bottom_up_proposals.py:188-191); ``load_proposal_file`` reads the file back."""
    with open(filename, 'w') as f:
        for i, rec in enumerate(records):
            f.write('# {}\n'.format(i + 1))
            f.write(rec)


def write_proposal_bytes(filename, data):
    """A list file whose bytes are complete already, '# <index>' lines included
    (``proposal_lists.ProposalListBuilder.build_text(...).data``): the file ``write_proposal_file`` writes from the same records."""
    with open(filename, 'wb') as f:
        f.write(data)


def format_processed_record(idx, frame_path, frame_cnt, gt, prop):
    """One record of a processed list (gt: [label, start, end] ints; prop: [label, iou, overlap_self, start, end])."""
    text = "# {}\n{}\n{}\n1\n{}\n".format(idx, frame_path, frame_cnt, len(gt))
    text += "".join("{} {:d} {:d}\n".format(*x) for x in gt)
    text += "{}\n".format(len(prop))
    text += "".join("{} {:.04f} {:.04f} {:d} {:d}\n".format(*x) for x in prop)
    return text


def process_proposal_list(norm_proposal_list, out_list_name, frame_dict):
    """Normalised list + ``frame_dict[vid] = (frame_path, frame_cnt, ...)`` -> processed list on disk."""
    records = []
    for idx, (vid, _, gt_boxes, pr_boxes) in enumerate(load_proposal_file(norm_proposal_list)):
        frame_path, frame_cnt = frame_dict[vid][0], frame_dict[vid][1]
        gt = [[int(x[0]), int(float(x[1]) * frame_cnt), int(float(x[2]) * frame_cnt)] for x in gt_boxes]
        prop = [[int(x[0]), float(x[1]), float(x[2]), int(float(x[3]) * frame_cnt), int(float(x[4]) * frame_cnt)]
                for x in pr_boxes]
        records.append(format_processed_record(idx, frame_path, frame_cnt, gt, prop))
    with open(out_list_name, 'w') as f:
        f.writelines(records)
