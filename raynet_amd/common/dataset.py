"""A dataset is a directory of scenes (raynet/common/dataset.py:8-103).

`RestrepoDataset`: every entry of the directory is a scene in Restrepo's layout, indexed by
alphabetical order.  `DTUDataset`: the directory is the DTU root, a scene index is a scan number
(`Rectified/scanNNN`).  Scenes are built on first use and cached; a DTU dataset keeps at most
`_max_cache_size` scans (the reference evicts a random one -- here the least recently used).
"""
import collections
import os

from .scene import DTUScene, RestrepoScene


class Dataset(object):
    def __init__(self, dataset_directory, select_neighbors_based_on="filesystem"):
        self._dataset_directory = dataset_directory
        self._cache = collections.OrderedDict()
        self._max_cache_size = 2
        self._select_neighbors_based_on = select_neighbors_based_on

    @property
    def n_scenes(self):
        return len(os.listdir(self._dataset_directory))

    @property
    def scenes(self):
        return sorted(os.listdir(self._dataset_directory))

    def get_scene(self, scene_idx):
        raise NotImplementedError()


class RestrepoDataset(Dataset):
    def __init__(self, dataset_directory, select_neighbors_based_on="filesystem"):
        super(RestrepoDataset, self).__init__(dataset_directory, select_neighbors_based_on)
        self._scene_mapping = dict(enumerate(self.scenes))

    def get_scene(self, scene_idx):
        if scene_idx not in self._scene_mapping:
            raise ValueError("scene_idx must be one of %r" % (sorted(self._scene_mapping),))
        if scene_idx not in self._cache:
            self._cache[scene_idx] = RestrepoScene(
                os.path.join(self._dataset_directory, self._scene_mapping[scene_idx]),
                select_neighbors_based_on=self._select_neighbors_based_on)
        return self._cache[scene_idx]


class DTUDataset(Dataset):
    def __init__(self, dataset_directory, illumination="max",
                 select_neighbors_based_on="filesystem"):
        super(DTUDataset, self).__init__(dataset_directory, select_neighbors_based_on)
        self._illumination = illumination

    @property
    def n_scenes(self):
        return len(os.listdir(os.path.join(self._dataset_directory, "Rectified")))

    @property
    def scenes(self):
        return sorted(os.listdir(os.path.join(self._dataset_directory, "Rectified")))

    def get_scene(self, scene_idx):
        if scene_idx in self._cache:
            self._cache.move_to_end(scene_idx)
            return self._cache[scene_idx]
        while len(self._cache) + 1 > self._max_cache_size:
            self._cache.popitem(last=False)
        self._cache[scene_idx] = DTUScene(self._dataset_directory, scene_idx, self._illumination,
                                          select_neighbors_based_on=self._select_neighbors_based_on)
        return self._cache[scene_idx]


def build_dataset(dataset_type, directory, illumination_condition="max",
                  select_neighbors_based_on="filesystem"):
    """scripts/arguments.py:448-464: "dtu" -> DTUDataset, anything else -> RestrepoDataset."""
    if dataset_type.lower() == "dtu":
        return DTUDataset(directory, illumination_condition,
                          select_neighbors_based_on=select_neighbors_based_on)
    return RestrepoDataset(directory, select_neighbors_based_on=select_neighbors_based_on)
