"""The dataset tree and the file readers on the host (reference dataloader/body.py, dataloader/heads/*).

dataset -> scenes -> agents -> files, the files of an agent sorted by the integer in the name; `pcd_range` prefix sums at
every level; `SlamDatasets.registration()` / `loop_detection()` select what an index means.  The names, the constructor
signatures and the order of every `random` call are the reference's, so a run seeded like the reference draws the same
frames.

What is added for the GPU loader (loader.py):

* every draw is split into a DRAW-ONLY form that returns a plan -- `plan_registration(index, rng)`,
  `plan_loop_detection(item, rng)` -- and a form that executes it (`execute_registration`, `execute_loop_detection`): the
  loader needs every file name of a batch before it reads the first byte.  `_getitem_registration` /
  `_getitem_loop_detection` keep the reference's interleaving (a map's frames are read and transformed before the next
  map's index is drawn);
* every draw takes an `rng` (Python's `random` module by default, a private `random.Random` in the seeded loader);
* every reader has `read_raw(path) -> (rows, stride, R, T, drop_nan)`: whole float32 records as they lie in the file,
  and the rule that decides which of them a frame keeps, for ops.ingest_frames to apply on the GPU.  `reader(path)`
  returns an `augment.PointCloud` as the reference's contract requires;
* `get_frame_dis` builds the pairwise distances in row chunks (peak host memory O(chunk x N), the reference's broadcast
  is O(N x N x 3)); the result is bit for bit the reference's.

`PcdReader` parses the PCD header itself (`DATA ascii` / `DATA binary`, x y z of F4 or F8, converted to float32 on the
host; `binary_compressed` raises NotImplementedError).  It is NOT pinned to open3d, which the reference reads .pcd files
with: open3d is not a dependency of this project.
"""
from __future__ import annotations

import logging
import os
import random
from glob import glob
from typing import Callable, Dict, List, Tuple, Union

import numpy as np
import torch
import torch.nn as nn
from torch.utils.data import Dataset

logger = logging.getLogger(__name__)

FRAME_DIS_CHUNK = 1024   # rows of frame_dis built at a time


# ------------------------------------------------------------------------------------------------------------
# readers (dataloader/heads/*.py)
# ------------------------------------------------------------------------------------------------------------
def filter_rows(rows: np.ndarray, drop_nan: bool) -> np.ndarray:
    """the rule `drop_nan` names, on the host: drop a record when one of its first three floats is NaN (heads/bin.py:16-17)"""
    return rows[np.isnan(rows[:, :3]).sum(1) == 0] if drop_nan else rows


def _records(a) -> np.ndarray:
    a = np.asarray(a)
    if a.ndim != 2 or a.shape[1] < 3:
        raise ValueError(f"a scan is (N, >=3), got {a.shape}")
    return np.ascontiguousarray(a, dtype=np.float32)


def _refuse(**extras):
    for name, v in extras.items():
        if v is not None:
            raise NotImplementedError(f"PointCloud({name}=...) is not carried by the GPU transforms")


class PointCloudReader:
    """heads/auto.py: the reader by file suffix.  Its .bin branch drops nothing (auto.py:41), unlike BinReader."""
    optional_type = ['npz', 'npy', 'bin']
    npz_extras = {'norm': 'lidar_norm', 'label': 'lidar_seg'}

    def __init__(self):
        pass

    def __call__(self, file_path: str):
        from .augment import PointCloud
        rows, _, rotation, translation, drop_nan = self.read_raw(file_path)
        return PointCloud(xyz=filter_rows(rows, drop_nan)[:, :3], rotation=rotation, translation=translation)

    def _type(self, file_path):
        file_type = os.path.splitext(file_path)[-1][1:]
        assert file_type in self.optional_type, f'Only type of the file in {self.optional_type} is optional, ' \
                                                f'not \'{file_type}\''
        return file_type

    def read_raw(self, file_path: str):
        """-> (rows (N,stride) float32 whole records, stride, R (3,3) | None, T (3,1) | None, drop_nan)"""
        file_type = self._type(file_path)
        if file_type == 'npy':
            return self._npy(file_path)
        if file_type == 'npz':
            return self._npz(file_path)
        if file_type == 'bin':
            return self._bin(file_path, drop_nan=False)
        raise ValueError(file_type)

    @staticmethod
    def _npy(file_path):
        rows = _records(np.load(file_path))
        return rows, rows.shape[1], None, None, False

    def _npz(self, file_path):
        with np.load(file_path, allow_pickle=True) as npz:
            keys = npz.files
            assert 'lidar_pcd' in keys, 'pcd file must contains \'lidar_pcd\''
            _refuse(**{name: (True if key in keys else None) for name, key in self.npz_extras.items()})
            rows = _records(npz['lidar_pcd'])
            rotation = npz['ego_rotation'] if 'ego_rotation' in keys else None
            translation = npz['ego_translation'] if 'ego_translation' in keys else None
        return rows, rows.shape[1], rotation, translation, False

    @staticmethod
    def _bin(file_path, drop_nan):
        rows = np.fromfile(file_path, dtype=np.float32).reshape(-1, 4)
        return rows, 4, None, None, drop_nan


class NPZReader(PointCloudReader):
    optional_type = ['npz']
    npz_extras = {'norm': 'lidar_norm', 'label': 'lidar_seg', 'image': 'image', 'uvd': 'lidar_proj'}

    def read_raw(self, file_path):
        self._type(file_path)
        return self._npz(file_path)


class NPYReader(PointCloudReader):
    optional_type = ['npy']

    def read_raw(self, file_path):
        self._type(file_path)
        return self._npy(file_path)


class BinReader(PointCloudReader):
    """heads/bin.py: records of four floats, the intensity column stays in `rows`; a record goes when x, y or z is NaN"""
    optional_type = ['bin']

    def read_raw(self, file_path):
        self._type(file_path)
        return self._bin(file_path, drop_nan=True)


_PCD_TYPES = {('F', 4): 'f4', ('F', 8): 'f8', ('I', 1): 'i1', ('I', 2): 'i2', ('I', 4): 'i4', ('I', 8): 'i8',
              ('U', 1): 'u1', ('U', 2): 'u2', ('U', 4): 'u4', ('U', 8): 'u8'}


def read_pcd_xyz(file_path: str) -> np.ndarray:
    """the x, y, z fields of a .pcd file (`DATA ascii` or `DATA binary`, F4 or F8) as (N,3) float32.  Not pinned to open3d."""
    with open(file_path, 'rb') as f:
        buf = f.read()
    hdr, pos, data = {}, 0, None
    while pos < len(buf):
        end = buf.find(b'\n', pos)
        end = len(buf) if end < 0 else end
        line = buf[pos:end].decode('ascii', errors='replace').strip()
        pos = end + 1
        if not line or line.startswith('#'):
            continue
        key, _, val = line.partition(' ')
        hdr[key.upper()] = val.split()
        if key.upper() == 'DATA':
            data = val.strip().lower()
            break
    if data is None or 'FIELDS' not in hdr:
        raise ValueError(f"'{file_path}' is not a PCD file (no FIELDS / DATA line)")
    if data == 'binary_compressed':
        raise NotImplementedError("PCD 'DATA binary_compressed' is not supported; convert the file to 'binary' or 'ascii'")
    if data not in ('ascii', 'binary'):
        raise ValueError(f"unknown PCD DATA kind '{data}'")
    fields = hdr['FIELDS']
    sizes = [int(v) for v in hdr.get('SIZE', ['4'] * len(fields))]
    types = [v.upper() for v in hdr.get('TYPE', ['F'] * len(fields))]
    counts = [int(v) for v in hdr.get('COUNT', ['1'] * len(fields))]
    if not (len(sizes) == len(types) == len(counts) == len(fields)):
        raise ValueError(f"'{file_path}': FIELDS / SIZE / TYPE / COUNT disagree")
    if 'POINTS' in hdr:
        n = int(hdr['POINTS'][0])
    else:
        n = int(hdr['WIDTH'][0]) * int(hdr.get('HEIGHT', ['1'])[0])
    for name in ('x', 'y', 'z'):
        if name not in fields:
            raise ValueError(f"'{file_path}' has no '{name}' field")
        k = fields.index(name)
        if types[k] != 'F' or sizes[k] not in (4, 8) or counts[k] != 1:
            raise NotImplementedError(f"PCD field '{name}' must be F4 or F8 with COUNT 1, got {types[k]}{sizes[k]} x {counts[k]}")
    if data == 'binary':
        dt = np.dtype([(f'{name}_{k}', '<' + _PCD_TYPES[(types[k], sizes[k])], (counts[k],) if counts[k] != 1 else ())
                       for k, name in enumerate(fields)])
        if len(buf) - pos < n * dt.itemsize:
            raise ValueError(f"'{file_path}' is truncated: {n} points of {dt.itemsize} bytes announced")
        rec = np.frombuffer(buf, dtype=dt, count=n, offset=pos)
        cols = [rec[f'{name}_{fields.index(name)}'] for name in ('x', 'y', 'z')]
    else:
        col0 = np.cumsum([0] + counts)
        tokens = buf[pos:].split()
        width = int(col0[-1])
        if len(tokens) < n * width:
            raise ValueError(f"'{file_path}' is truncated: {n} points of {width} values announced")
        table = np.array(tokens[:n * width], dtype=object).reshape(n, width)
        cols = [np.array([float(v) for v in table[:, col0[fields.index(name)]]], dtype=np.float64) for name in ('x', 'y', 'z')]
    return np.stack([c.astype(np.float32) for c in cols], axis=1) if n else np.zeros((0, 3), np.float32)


class PcdReader(PointCloudReader):
    """heads/pcd.py without open3d (module docstring): x, y, z converted to float32 on the host; a point goes when x, y or
    z is NaN (pcd.py:19)"""
    optional_type = ['pcd']

    def read_raw(self, file_path):
        self._type(file_path)
        return read_pcd_xyz(file_path), 3, None, None, True


READER: Dict[str, type] = {
    'auto': PointCloudReader,
    'npz': NPZReader,
    'npy': NPYReader,
    'bin': BinReader,
    'pcd': PcdReader,
}


def get_length_range(l):
    length_range = [0]
    for i in l:
        length_range.append(len(i) + length_range[-1])
    return length_range


# ------------------------------------------------------------------------------------------------------------
# the tree (dataloader/body.py)
# ------------------------------------------------------------------------------------------------------------
class SlamDatasets(Dataset):

    def __init__(self, args, data_transforms: Callable = nn.Identity()):
        Dataset.__init__(self)
        self.args = args
        self.dataset_cfg = self.args.dataset
        self.registration_cfg = self.args.train.registration
        self.loop_detection_cfg = self.args.train.loop_detection
        self.data_transforms = data_transforms

        self.dataset_list = self.load_dataset()  # [BasicDataset1, BasicDataset2, ...]

        self.pcd_range = get_length_range(self.dataset_list)
        self.pcd_range = torch.tensor(self.pcd_range, dtype=torch.int32)

        self.frame_distance = get_frame_dis(self.dataset_list)

        self._getitem_method = self._getitem_registration
        self.collate_fn = self.map_collate_fn
        self.stage = 'registration'

    def __getitem__(self, item):
        return self._getitem_method(item)

    # ---- where an index lives
    def _locate(self, index):
        """index -> (dataset_id, dataset, offset in the dataset, scene_id, frame offset in the scene, frame_dis row)"""
        dataset_id = (torch.sum(self.pcd_range <= index) - 1).item()
        offset = index - self.pcd_range[dataset_id]
        curren_dataset = self.dataset_list[dataset_id]
        scene_id, frame_offset = curren_dataset.get_frame_order(offset)
        frame_dis = self.frame_distance[dataset_id][scene_id][frame_offset]
        return dataset_id, curren_dataset, int(offset), scene_id, frame_offset, frame_dis

    # ---- loop detection (body.py:62-95)
    def plan_loop_detection(self, item, rng=random) -> dict:
        """the draws of _getitem_loop_detection, nothing read: {'files': (first, second), 'items': their dataset offsets}"""
        dataset_id, curren_dataset, offset, scene_id, frame_offset, frame_dis = self._locate(item)
        s = rng.random()
        d = self.loop_detection_cfg.distance
        if s < 0.5:
            dis_mask = frame_dis <= d
        elif s < 0.75:
            dis_mask = (frame_dis > d) & (frame_dis <= 2 * d)
        else:
            dis_mask = frame_dis > 2 * d
        optional_pair_offset = torch.nonzero(dis_mask).squeeze(1) - frame_offset
        optional_pair_offset = optional_pair_offset.tolist()
        if len(optional_pair_offset) > 0:
            pair_offset = rng.choice(optional_pair_offset)
        else:
            pair_offset = 0
        return dict(dataset_id=dataset_id, items=(offset, offset + pair_offset),
                    files=(curren_dataset.file_of(offset), curren_dataset.file_of(offset + pair_offset)))

    def execute_loop_detection(self, plan: dict):
        curren_dataset = self.dataset_list[plan['dataset_id']]
        frame1 = curren_dataset[plan['items'][0]]      # loaded before the second, transformed after it: body.py:69,92-94
        frame2 = curren_dataset[plan['items'][1]]
        frame1 = self.data_transforms(frame1)
        frame2 = self.data_transforms(frame2)
        return *frame1, *frame2

    def _getitem_loop_detection(self, item, rng=random):
        return self.execute_loop_detection(self.plan_loop_detection(item, rng))

    # ---- registration (body.py:97-153)
    def _draw_maps(self, rng):
        S = rng.randint(2, self.registration_cfg.K)
        if rng.random() < 0.34:
            S = 2
        if self.registration_cfg.fill:
            num_map = self.registration_cfg.K_max // S
        else:
            num_map = 1
        return S, num_map, dict(dsf_index=[], refined_SE3_file=[], num_map=num_map)

    def plan_registration(self, index: int, rng=random) -> dict:
        """the draws of _getitem_registration, nothing read: {'S', 'num_map', 'frames': [(dataset, scene, frame, file), ...]
        in reading order, 'info'}.  (With a transform that draws from the same `rng`, _getitem_registration interleaves
        those draws with these, map by map, as the reference does; the loader plans first.)"""
        S, num_map, info = self._draw_maps(rng)
        frames = []
        for i in range(num_map):
            frames += self._plan_map_query(index if i == 0 else rng.randint(0, self.__len__() - 1), K=S, info=info, rng=rng)
        return dict(S=S, num_map=num_map, frames=frames, info=info)

    def execute_registration(self, plan: dict) -> Tuple[List, dict]:
        return [self._frame(d, s, f) for d, s, f, _ in plan['frames']], plan['info']

    def _frame(self, dataset_id, scene_id, frame_index):
        frame = self.dataset_list[dataset_id].scene_list[scene_id][frame_index]
        return self.data_transforms(frame)

    def _getitem_registration(self, index: int, rng=random) -> Tuple[List, dict]:
        S, num_map, info = self._draw_maps(rng)
        frame_list = []
        for i in range(num_map):
            if i == 0:
                frame_list += self._map_query(index, K=S, info=info, rng=rng)
            else:
                rand_index = rng.randint(0, self.__len__() - 1)
                frame_list += self._map_query(rand_index, K=S, info=info, rng=rng)
        return frame_list, info

    def _plan_map_query(self, index: int, K: int, info: dict, rng=random) -> List[tuple]:
        dataset_id, curren_dataset, offset, scene_id, frame_offset, frame_dis = self._locate(index)

        dis_mask = frame_dis <= self.registration_cfg.distance - 0.25
        optional_frame_offsets = torch.nonzero(dis_mask).squeeze(1) - frame_offset
        optional_frame_offsets = optional_frame_offsets.tolist()
        optional_frame_offsets.remove(0)
        if dis_mask.sum() <= K:
            if len(optional_frame_offsets) == 0:
                optional_frame_offsets.append(0)
            optional_frame_offsets = optional_frame_offsets * (K // len(optional_frame_offsets) + 1)
        map_frame_offsets = rng.sample(optional_frame_offsets, k=K - 1)
        map_frame_offsets.insert(0, 0)
        info['dsf_index'] += [(dataset_id, scene_id, frame_offset + off) for off in map_frame_offsets]
        if 'carla' in curren_dataset.name.lower():
            refined_SE3_file = ''
        else:
            refined_SE3_file = os.path.join(curren_dataset.scene_list[scene_id].root, 'refined_SE3.pkl')
        info['refined_SE3_file'].append(refined_SE3_file)
        scene = curren_dataset.scene_list[scene_id]
        return [(dataset_id, scene_id, frame_offset + off, scene.file_of(frame_offset + off)) for off in map_frame_offsets]

    def _map_query(self, index: int, K: int, info: dict, rng=random) -> List:
        return [self._frame(d, s, f) for d, s, f, _ in self._plan_map_query(index, K, info, rng)]

    @staticmethod
    def map_collate_fn(batch):
        frame_list, info = batch[0]
        batch_data_list = []
        for data in zip(*frame_list):
            batch_data_list.append(torch.stack(data, dim=0))
        return *batch_data_list, info

    def __len__(self):
        return int(self.pcd_range[-1])

    def load_dataset(self):
        dataset_list: List[BasicDataset] = []
        for dataset_dict in self.dataset_cfg:
            name = dataset_dict.name
            root = dataset_dict.root
            scenes = dataset_dict.scenes
            reader_cfg = dataset_dict.reader
            reader = READER[reader_cfg.type](**reader_cfg.get('kwargs', {}))
            basic_dataset = BasicDataset(root=root, reader=reader, scenes=scenes, name=name.lower(), args=self.args)
            dataset_list.append(basic_dataset)
            logger.info(f'Load {name} successfully: \'{basic_dataset.root}\'')
        return dataset_list

    def get_seq_range(self):
        real_range = [0]
        for dataset in self.dataset_list:
            for scene in dataset.scene_list:
                for agent in scene.agent_list:
                    real_range.append(len(agent) + real_range[-1])
        return torch.tensor(real_range, dtype=torch.int32)

    def get_datasets(self):
        return self.dataset_list

    @property
    def seq_begin_list(self):
        return self.get_seq_range()

    def get_data_source(self, item):
        dataset_id = torch.sum(self.pcd_range <= item) - 1
        return self.dataset_list[dataset_id]

    def registration(self):
        self._getitem_method = self._getitem_registration
        self.collate_fn = self.map_collate_fn
        self.stage = 'registration'

    def loop_detection(self):
        self._getitem_method = self._getitem_loop_detection
        self.collate_fn = None
        self.stage = 'loop_detection'

    def __repr__(self):
        return self.__str__()

    def __str__(self):
        my_str = ''
        my_str += ('=' * 50 + '\n')
        my_str += (f'SlamDatasets: num_datasets={len(self.dataset_list)}\n'
                   f'    |\n')
        for dataset in self.dataset_list:
            my_str += (f'    |——{dataset.name}\n'
                       f'    |   |——train: num_scenes={len(dataset.scene_list)} | num_frames={dataset.pcd_range[-1]}\n'
                       f'    |\n')
        my_str += ('=' * 50)
        return my_str


class BasicDataset:
    """
    dataset
        |--scenes
             |--00
             |--01
             |--02
                 |--agent 0
                 |--agent 1
                 |--agent 2
                        |--0.npz
                        |--1.npz
                        |--2.npz
    """

    def __init__(self, args, root: str, reader, scenes: list, name: str):
        self.args = args
        self.root = root
        self.scenes = scenes
        self.name = name

        if not isinstance(self.root, str) or not os.path.isdir(self.root):
            raise NotADirectoryError(f'\'{self.root}\' is not a directory')

        self.scene_list: List[BasicScene] = []
        for scene_name in self.scenes:
            scene_root = os.path.join(self.root, scene_name)
            if not os.path.isdir(scene_root):
                raise NotADirectoryError(f'\'{scene_root}\' is not a directory')
            self.scene_list.append(BasicScene(root=scene_root, reader=reader, parent=self, args=self.args))
        self.pcd_range = get_length_range(self.scene_list)
        self.pcd_range = torch.tensor(self.pcd_range, dtype=torch.int32)

    def __getitem__(self, item):
        scene_id = torch.sum(self.pcd_range <= item) - 1
        offset = item - self.pcd_range[scene_id]
        return self.scene_list[scene_id][offset]

    def file_of(self, item) -> str:
        scene_id, offset = self.get_frame_order(item)
        return self.scene_list[scene_id].file_of(offset)

    def read_raw(self, item):
        scene_id, offset = self.get_frame_order(item)
        return self.scene_list[scene_id].read_raw(offset)

    def __len__(self):
        return int(self.pcd_range[-1])

    def get_scenes(self):
        return self.scene_list

    def get_frame_order(self, item):
        scene_id = torch.sum(self.pcd_range <= item) - 1
        offset = item - self.pcd_range[scene_id]
        return scene_id.item(), int(offset)


class BasicScene:

    def __init__(self, args, root: str, reader, parent: BasicDataset):
        self.root = root
        self.args = args
        self.parent = parent

        self.agent_list: List[BasicAgent] = []
        for agent_name in sorted(os.listdir(self.root)):
            agent_root = os.path.join(self.root, agent_name)
            if os.path.isdir(agent_root):
                self.agent_list.append(BasicAgent(root=agent_root, reader=reader, parent=self))

        self.pcd_range = get_length_range(self.agent_list)
        self.pcd_range = torch.tensor(self.pcd_range, dtype=torch.int32)

    def _order(self, item):
        agent_id = torch.sum(self.pcd_range <= item) - 1
        return int(agent_id), int(item - self.pcd_range[agent_id])

    def __getitem__(self, item):
        agent_id, offset = self._order(item)
        return self.agent_list[agent_id][offset]

    def file_of(self, item) -> str:
        agent_id, offset = self._order(item)
        return self.agent_list[agent_id].file_list[offset]

    def read_raw(self, item):
        """the records of frame `item` as its agent's reader finds them (PointCloudReader.read_raw)"""
        agent_id, offset = self._order(item)
        agent = self.agent_list[agent_id]
        return agent.reader.read_raw(agent.file_list[offset])

    def __len__(self):
        return int(self.pcd_range[-1])


class BasicAgent(Dataset):

    def __init__(self, root: str, reader: Union[PointCloudReader, str], parent: BasicScene = None, split_num: int = 1,
                 split_index: int = 0):
        Dataset.__init__(self)
        self.root = root
        self.reader = reader
        self.parent = parent
        self.data_transforms = None
        file_name_list = glob(os.path.join(self.root, '*.*'))
        file_type = set([os.path.splitext(i)[1] for i in file_name_list])
        assert len(file_type) <= 1, 'The root can only contain files of the SAME type'
        file_type = file_type.pop()[1:]
        if self.reader == 'auto':
            self.reader = READER[file_type]()
        file_name_list = sorted(file_name_list, key=lambda s: int(os.path.basename(s).split('.')[0]))

        if split_num > 1:
            total_len = len(file_name_list)
            agent_ratio = 1 / split_num
            overlap_ratio = 1 / 20  # 5% overlapped frames
            start_ratio = max(agent_ratio * split_index - overlap_ratio, 0.0)
            end_ratio = min(agent_ratio * (split_index + 1) + overlap_ratio, 1.0)
            self.file_list = file_name_list[int(total_len * start_ratio):int(total_len * end_ratio)]
        else:
            self.file_list = file_name_list

    def __getitem__(self, item):
        data = self.reader(self.file_list[item])
        if self.data_transforms is not None:
            data = self.data_transforms(data)
        return data

    def __len__(self):
        return len(self.file_list)

    def set_independent(self, data_transforms: Callable):
        self.data_transforms = data_transforms


# ------------------------------------------------------------------------------------------------------------
# frame distances (body.py:363-396)
# ------------------------------------------------------------------------------------------------------------
def pairwise_frame_dis(frame_poses: np.ndarray, chunk: int = FRAME_DIS_CHUNK) -> np.ndarray:
    """(N,3) float32 -> (N,N) float32 distances, `chunk` rows at a time: the bits of the reference's one-shot
    np.linalg.norm(poses[:, None] - poses[None], ord=2, axis=-1), which is sqrt((dx*dx + dy*dy) + dz*dz) in float32 per
    element whatever the slicing."""
    n = frame_poses.shape[0]
    out = np.empty((n, n), dtype=np.float32)
    chunk = max(int(chunk), 1)
    for r0 in range(0, n, chunk):
        diff = np.expand_dims(frame_poses[r0:r0 + chunk], axis=1) - np.expand_dims(frame_poses, axis=0)
        out[r0:r0 + chunk] = np.linalg.norm(x=diff, ord=2, axis=-1)
    return out


def get_frame_dis(dataset_list: List[BasicDataset], chunk: int = FRAME_DIS_CHUNK) -> List[List[torch.Tensor]]:
    """per dataset, per scene: the (N,N) half-precision distances between the frames' `ego_translation`.  Cached as
    `frame_dis.npy` in the scene's directory: loaded when it is square and matches the frame count, else built and saved."""
    frame_distance = []
    for i, dataset in enumerate(dataset_list):
        dataset_frame_dis = []
        for j, scene in enumerate(dataset.scene_list):
            frame_files = []
            for agent in scene.agent_list:
                frame_files += agent.file_list

            frame_dis_file = os.path.join(scene.root, 'frame_dis.npy')
            cache_right = False
            if os.path.exists(frame_dis_file):
                frame_dis: np.ndarray = np.load(frame_dis_file).astype(np.float32)
                if frame_dis.ndim == 2 and frame_dis.shape[0] == frame_dis.shape[1] == len(frame_files):
                    cache_right = True
            if not cache_right:
                frame_poses = []
                for frame_file in frame_files:
                    with np.load(frame_file, allow_pickle=True) as npz:
                        frame_poses.append(npz['ego_translation'].squeeze(1).astype(np.float32))  # (3, 1), f32
                frame_poses = np.stack(frame_poses, axis=0)  # (N, 3)
                frame_dis = pairwise_frame_dis(frame_poses, chunk)
                np.save(file=frame_dis_file, arr=frame_dis)
                logger.info(f'File \'frame_dis\' has been saved in {frame_dis_file}')

            frame_dis = torch.from_numpy(frame_dis).half()
            dataset_frame_dis.append(frame_dis)
        frame_distance.append(dataset_frame_dis)
    return frame_distance
