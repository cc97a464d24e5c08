// Camera kinds and the angular camera's projections (DevCamera::kind / ::projection): shared by the host's staging
// (devscene.h) and by camera.h's ray functions, which a host program compiles without the HIP headers.
#pragma once

namespace yafamd
{

// (the architect camera is a perspective camera with another vup: host.cc)
enum CameraKind : int { CAM_PERSPECTIVE = 0, CAM_ORTHO = 1, CAM_EQUIRECT = 2, CAM_ANGULAR = 3 };
// camera_angular.h Projection
enum AngularProjection : int { AP_EQUIDISTANT = 0, AP_ORTHOGRAPHIC = 1, AP_STEREOGRAPHIC = 2, AP_EQUISOLID = 3, AP_RECTILINEAR = 4 };

} // namespace yafamd
