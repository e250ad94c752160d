"""stlpose_amd -- MI355X-native HRNet / perceptual-loss hot path (drop-in for STLPose's
``models.PoseHighResolutionNet`` and the per-batch functions of ``lib/``)."""
from .hrnet import PoseHighResolutionNet  # noqa: F401,E402
from .loss import PersonMSELoss, apply_perceptual_loss  # noqa: F401,E402
from .inference import forward_pass  # noqa: F401,E402
from .pose_parsing import get_max_preds_hrnet, get_final_preds_hrnet, accuracy  # noqa: F401,E402
from .vgg import VGGPerceptualLoss  # noqa: F401,E402
from .vgg19_style import VGG19StyleLoss  # noqa: F401,E402
from .stylise import GatysStylizer  # noqa: F401,E402
from .pose_database import (PoseIndex, process_pose_vector, process_pose_vectors, get_neighbors_idxs,  # noqa: F401,E402
                            get_penalization_metric, fit_knn_structure, load_knn)
from .retrieval import score_retrievals, retrieval_experiment, process_retrieval_results  # noqa: F401,E402
from .pose_parsing import create_pose_entries, create_pose_from_outputs  # noqa: F401,E402
from .bounding_box import (bbox_filtering, bbox_nms, get_detections, reshape_detection,  # noqa: F401,E402
                           bbox_to_image_keypoints)
from .topdown import TransformDetection, PoseExtractor, extract_retrieval_db  # noqa: F401,E402
from .efficientdet import EfficientDetBackbone, EfficientDet, setup_detector  # noqa: F401,E402
from .topdown import detect_poses  # noqa: F401,E402
from .adain import AdaINStylizer  # noqa: F401,E402
from .styled_coco import create_styled_dataset  # noqa: F401,E402
from .detection_eval import box_ap, CocoEvaluator, DetectorEvaluator  # noqa: F401,E402
from .detections import Detections, DetectionStore  # noqa: F401,E402
from .keypoint_eval import keypoint_ap, keypoint_ap_tables, rescore_and_nms_device, KeypointGroundTruth, PoseResults  # noqa: F401,E402
from .eval_tail import EvalTables  # noqa: F401,E402
from .pose_parsing import pck_from_coords  # noqa: F401,E402
from .pose_data import coco_person_db, epoch_indices, ResidentImages, StreamedImages, PoseBatchLoader, PersonDB  # noqa: F401,E402
from .det_data import coco_detection_db, DetectionDB, DetBatch, DetBatchLoader  # noqa: F401,E402
from .detector_trainer import DetectorTrainer  # noqa: F401,E402
