"""Annotation readers for THUMOS14 and ActivityNet: the video records the proposal-list stage starts from (host only).

They follow the rules of the reference's /root/reference/ops/thumos_db.py:136-242 and ops/anet_db.py:137-203, so that the
label indices and the order of videos and instances -- and with them every line of a proposal list -- are the reference's.
The annotation location is an argument: the repository ships no data set.

    db = ThumosDB.from_folder("data/thumos_14")          # or ANetDB.from_json("data/activity_net.v1-3.min.json")
    db.try_load_file_path("/data/thumos14_frames")
    videos = db.get_subset_videos("test")

One choice the reference leaves to the file system is fixed here: it reads the THUMOS class files in the order ``glob``
lists them, which decides the order of a video's instances; this reader takes them in alphabetical order.
"""
import glob
import json
import os


class Instance(object):
    """One annotated action: ``num_label`` (index into the ordered label list), ``label`` (its name) and ``time_span``
    (start, end) in seconds."""

    def __init__(self, video_id, index, label, num_label, start, end):
        self.name = "{}_{}".format(video_id, index)
        self.label = label
        self.num_label = num_label
        self.time_span = (start, end)

    def __repr__(self):
        return "Instance(%s, %s, %r)" % (self.name, self.label, self.time_span)


class Video(object):
    """One video: ``id``, ``duration`` (seconds), ``subset``, ``instances``.  ``path`` is the frame folder and raises until
    ``try_load_file_path`` (or an assignment) has attached one."""

    def __init__(self, video_id, duration, subset, annotations, name_to_index):
        self.id = video_id
        self.duration = duration
        self.subset = subset
        self.instances = [Instance(video_id, i, label, name_to_index.get(label), start, end)
                          for i, (label, start, end) in enumerate(annotations)]
        self._path = None

    @property
    def path(self):
        if self._path is None:
            raise ValueError("video {} has no frame folder attached (is it missing under the frame path?)".format(self.id))
        return self._path

    @path.setter
    def path(self, value):
        self._path = value

    def __repr__(self):
        return "Video(%s, %r s, %d instances)" % (self.id, self.duration, len(self.instances))


class _Database(object):
    """What the two readers share: subsets of Video records, the ordered label list, attaching frame folders."""

    subsets = ()

    def __init__(self):
        self._subset_videos = {}          # subset -> {id: Video}, in the subset's order
        self._labels = []

    def get_subset_videos(self, subset):
        if subset not in self._subset_videos:
            raise ValueError("Unknown subset {} (this database has {})".format(subset, ", ".join(self.subsets)))
        return list(self._subset_videos[subset].values())

    def get_subset_instance(self, subset):
        return [i for v in self.get_subset_videos(subset) for i in v.instances]

    def get_ordered_label_list(self):
        return list(self._labels)

    @staticmethod
    def folder_key(name):
        raise NotImplementedError

    def try_load_file_path(self, frame_path):
        """Attach the folders under ``frame_path`` to the videos whose id is the folder's key; -> how many were attached.
        Of two folders with one key the later in alphabetical order wins."""
        folders = sorted(glob.glob(os.path.join(frame_path, "*")))
        by_key = {self.folder_key(f): f for f in folders}
        count = 0
        for videos in self._subset_videos.values():
            for vid, video in videos.items():
                if vid in by_key:
                    video.path = by_key[vid]
                    count += 1
        return count


class ThumosDB(_Database):
    """THUMOS14 from the layout of the reference's ``data/thumos_14``: ``{validation,test}_durations.txt`` (name and
    duration on alternating lines), ``temporal_annotations_{validation,test}/<Class>_*.txt`` (``video start end`` per
    line) and ``{validation,test}_avoid_videos.txt`` (``video Class`` per line)."""

    subsets = ("validation", "test")
    ignore_labels = ("Ambiguous",)

    @classmethod
    def from_folder(cls, folder):
        me = cls()
        loaded = {s: me._load_subset(folder, s) for s in cls.subsets}
        names = {s: sorted(c for c, _ in loaded[s][1]) for s in cls.subsets}
        if names["validation"] != names["test"]:
            raise IOError("validation and test annotations name different classes: {} v.s. {}".format(
                names["validation"], names["test"]))
        me._labels = sorted(c for c in names["validation"] if c not in cls.ignore_labels)
        index = {c: i for i, c in enumerate(me._labels)}
        for s in cls.subsets:
            info, class_files = loaded[s][0], loaded[s][1]
            avoid = loaded[s][2]
            table = {name: [] for name, _ in info}
            durations = dict(info)
            for cls_name, path in class_files:
                with open(path) as f:
                    for line in f:
                        items = line.split()
                        if not items:
                            continue
                        vid, start, end = items[0], float(items[1]), float(items[2])
                        if vid not in durations:
                            raise ValueError("{}: annotation of {}, which {}_durations.txt does not list".format(path, vid, s))
                        # an avoided (video, class) pair is dropped, and so is an instance that starts behind the video's end
                        if (vid, cls_name) not in avoid and start <= float(durations[vid]):
                            table[vid].append((cls_name, start, end))
            me._subset_videos[s] = {
                name: Video(name, float(duration), s, [a for a in table[name] if a[0] not in cls.ignore_labels], index)
                for name, duration in info}
        return me

    @staticmethod
    def _load_subset(folder, subset):
        with open(os.path.join(folder, "{}_durations.txt".format(subset))) as f:
            lines = [x.strip() for x in f]
        info = [(lines[i].split(".")[0], lines[i + 1]) for i in range(0, len(lines) - 1, 2)]
        files = glob.glob(os.path.join(folder, "temporal_annotations_{}".format(subset), "*"))
        class_files = [(os.path.basename(p).split("_")[0], p) for p in sorted(files)]
        with open(os.path.join(folder, "{}_avoid_videos.txt".format(subset))) as f:
            avoid = set(tuple(x.split()) for x in f if x.strip())
        return info, class_files, avoid

    @staticmethod
    def folder_key(name):
        return os.path.split(name)[-1]


class ANetDB(_Database):
    """ActivityNet from its release JSON (``taxonomy`` + ``database``): the classes are the leaf nodes of the taxonomy in
    alphabetical order, every subset is ordered by video id."""

    subsets = ("training", "validation", "testing")

    @classmethod
    def from_json(cls, path):
        with open(path) as f:
            raw = json.load(f)
        me = cls()
        me.version = raw.get("version")
        nodes = set(x["nodeName"] for x in raw["taxonomy"])
        parents = set(x["parentName"] for x in raw["taxonomy"])
        me._labels = sorted(nodes - parents)          # a leaf is a node that is nobody's parent
        index = {c: i for i, c in enumerate(me._labels)}
        for s in cls.subsets:
            me._subset_videos[s] = {
                k: Video(k, v["duration"], s, [(a["label"], a["segment"][0], a["segment"][1]) for a in v["annotations"]], index)
                for k, v in sorted(raw["database"].items()) if v["subset"] == s}
        return me

    @staticmethod
    def folder_key(name):
        return os.path.splitext(name)[0][-11:]


def open_database(dataset, annotations):
    """The reader of ``dataset`` ('thumos14' / 'activitynet') on the annotations at ``annotations``."""
    if dataset == "thumos14":
        return ThumosDB.from_folder(annotations)
    if dataset == "activitynet":
        return ANetDB.from_json(annotations)
    raise ValueError("Unknown dataset {}".format(dataset))
